// graph_lm.h -- the Ceres-rule Levenberg-Marquardt loop on a graph whose nodes are 3-vectors and whose edges carry
// three residuals between two nodes (nonlinear_rotations.hip: views and PairwiseRotationError; nonlinear_positions.hip:
// views and track points and PairwiseTranslationError).  A stage writes one 24-double record per edge,
// J_i [3][3] | J_j [3][3] | r [3] | 3 unused, the loss corrector and the Jacobi scaling applied, in a k_linearise of its
// own, and evaluates the candidate in a k_candidate of its own; everything downstream of the record is here:
//   k_column_norms  first linearisation only, one wavefront per free node: scale = 1 / (1 + |column|)
//   k_gradient    one wavefront per free node: Js' r over its incident edges; max |g| per block
//   k_post        one workgroup: gradient max norm, the trace row, then cap / gradient tolerance / radius floor
//   k_assemble    lower triangle of Js'Js + D and the right-hand-side row, owner sums in edge order (view_graph_plan.h)
//   k_step        one lane per free node: candidate x - scale * y, |step|^2 and |candidate|^2 per block
//   k_decide      one workgroup: Ceres' rules in Ceres' order; swaps the iterate on acceptance; raises `done`
// DESIGN.md 3.3 has the rules, 3.6i the loop, 3.6j what is shared.  The kernels sit in an unnamed namespace: every file
// that includes this header compiles its own copies, under its own flags.  No atomics; every sum has one owner and a
// fixed order.
#pragma once
#include "dense_cholesky.h"
#include "lm_rules.h"
#include "view_graph_device.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

namespace thip {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == 64 * kViewsPerBlock, "k_column_norms, k_gradient: one wavefront per free view");
constexpr int kRec = 24;                        // doubles per edge record: J_i [3][3] | J_j [3][3] | r [3] | 3 unused
constexpr int kDefaultChunk = 4;                // LM iterations enqueued between two reads of the state
constexpr int kMaxChunk = 64;

struct NlState {
  int done, term, iterations, successful, unsuccessful, invalid;
  int invalid_steps;     // consecutive invalid steps
  int step_successful;   // the last step was accepted (the gradient rule applies after successful steps only)
  int fresh;             // the iterate changed: k_linearise / k_gradient run, k_post takes the new gradient
  int trace_rows, pad0, pad1;
  double cost, initial_cost, gmax, x_norm, radius, decrease_factor;   // (with the two ints above: the state of lm_rules.h)
};

// The first linearisation ran with scale = 1; one wavefront per free view sums the squares of its three columns over its
// incident edges (lane l takes edges l, l + 64, .. in order, then the butterfly) and writes scale = 1 / (1 + |column|).
__global__ __launch_bounds__(kThreads) void k_column_norms(ViewGraphLists vg, const double* __restrict__ rec,
                                                           double* __restrict__ scale) {
  const int v = blockIdx.x * kViewsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= vg.m) return;   // wave-uniform
  double s[3] = {0.0, 0.0, 0.0};
  for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
    const double* J = rec + kRec * (size_t)e + 9 * (int)plus;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (J[c] * J[c] + J[3 + c] * J[3 + c]) + J[6 + c] * J[6 + c];
  });
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = wave_sum_butterfly(s[c]);
    if (lane == 0) scale[3 * (size_t)v + c] = lm::jacobi_scale(t);
  }
}

// g = Js' r, one wavefront per free view as above; part_g[block] = max |g / scale| over the workgroup's views (the
// gradient of the unscaled problem, which the gradient tolerance is about).
__global__ __launch_bounds__(kThreads) void k_gradient(ViewGraphLists vg, const double* __restrict__ rec,
                                                       const double* __restrict__ scale, double* __restrict__ g,
                                                       double* __restrict__ part_g, const NlState* __restrict__ st) {
  __shared__ double red[kViewsPerBlock];
  if (st->done || !st->fresh) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.x * kViewsPerBlock + wv;
  double gm = 0.0;
  if (v < vg.m) {   // wave-uniform
    double s[3] = {0.0, 0.0, 0.0};
    for_each_incident_edge(vg, v, lane, [&](int e, bool plus) {
      const double* R = rec + kRec * (size_t)e;
      const double* J = R + 9 * (int)plus;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += (J[c] * R[18] + J[3 + c] * R[19]) + J[6 + c] * R[20];
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = wave_sum_butterfly(s[c]);
      if (lane == 0) g[3 * (size_t)v + c] = t;
      gm = fmax(gm, fabs(t / scale[3 * (size_t)v + c]));
    }
  }
  if (lane == 0) red[wv] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0];
    for (int k = 1; k < kViewsPerBlock; ++k) a = fmax(a, red[k]);
    part_g[blockIdx.x] = a;
  }
}

__device__ __forceinline__ void trace_row(double* trace, int capacity_rows, NlState* st, double cost, double gmax,
                                          double step, double radius, int accepted) {
  if (st->trace_rows < capacity_rows) {
    double* t = trace + 5 * (size_t)st->trace_rows;
    t[0] = cost; t[1] = gmax; t[2] = step; t[3] = radius; t[4] = (double)accepted;
  }
  st->trace_rows += 1;
}

// One workgroup, after every k_decide and once at the start (init = 1).  When the iterate is fresh: the gradient max norm
// of the new linearisation (at the start also the cost, |x| and trace row 0) goes into the state and the trace.  Then
// the rules that end the loop between two iterations, in Ceres' order: at the start the gradient tolerance, then the cap;
// afterwards the cap, the gradient tolerance (after a successful step only), the radius floor.
__global__ __launch_bounds__(kThreads) void k_post(int init, int m, const int* __restrict__ free_view,
                                                   const double* __restrict__ x, const double* __restrict__ part_cost, int nbE,
                                                   const double* __restrict__ part_g, int nbV, int max_iterations,
                                                   double gradient_tolerance, double* __restrict__ trace,
                                                   int capacity_rows, int term_gradient, int term_cap, int term_radius,
                                                   NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  __shared__ int flags[2];
  if (threadIdx.x == 0) { flags[0] = st->done; flags[1] = st->fresh; }
  __syncthreads();
  if (flags[0]) return;
  const bool fresh = flags[1] != 0;
  double gmax = 0.0, cost = 0.0, xn = 0.0;
  if (fresh) {
    double a = 0.0;
    for (int k = threadIdx.x; k < nbV; k += kThreads) a = fmax(a, part_g[k]);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
      __syncthreads();
    }
    gmax = red[0];
    __syncthreads();
    if (init) {
      double q = 0.0;
      for (int k = threadIdx.x; k < m; k += kThreads) {
        const double* w = x + 3 * (size_t)free_view[k];
        q += (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
      }
      cost = block_sum_column<kThreads>(part_cost, nbE, 1, 0, red);
      xn = block_sum<kThreads>(q, red);
    }
  }
  if (threadIdx.x != 0) return;
  if (fresh) {
    st->gmax = gmax;
    if (init) {
      st->cost = st->initial_cost = 0.5 * cost;
      st->x_norm = sqrt(xn);
      trace_row(trace, capacity_rows, st, st->cost, gmax, 0.0, st->radius, 1);
    } else if (st->trace_rows - 1 < capacity_rows) {
      trace[5 * (size_t)(st->trace_rows - 1) + 1] = gmax;
    }
    st->fresh = 0;
  }
  const bool grad = st->step_successful && st->gmax <= gradient_tolerance;   // lm::gradient_rule, written out (2 registers)
  const bool cap = st->iterations >= max_iterations;
  if (init && grad) { st->done = 1; st->term = term_gradient; }
  else if (cap) { st->done = 1; st->term = term_cap; }
  else if (grad) { st->done = 1; st->term = term_gradient; }
  else if (lm::radius_floor(*st)) { st->done = 1; st->term = term_radius; }
}

// The lower triangle of Js'Js + D into the cleared array (row-major, leading dimension lda), D = clamp(diag(Js'Js), 1e-6,
// 1e32) / radius, and g into row 3m, the factorisation's right-hand-side row:
//   thread t < m       : free view t -- its 3 x 3 diagonal block, sum of J' J over its incident edges, and its part of g
//   thread t = m + p   : pair p = (a > b) -- block (a, b) = sum of J_a' J_b over the pair's edges
__global__ __launch_bounds__(kThreads) void k_assemble(ViewGraphLists vg, int lda, const double* __restrict__ rec,
                                                       const double* __restrict__ g, double* __restrict__ A,
                                                       const NlState* __restrict__ st) {
  if (st->done) return;
  const int t = blockIdx.x * kThreads + threadIdx.x, m = vg.m;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < m) {
    for (int k = vg.inc_off[t]; k < vg.inc_off[t + 1]; ++k) {
      const double* J = rec + kRec * (size_t)(vg.inc[k] >> 1) + 9 * (vg.inc[k] & 1);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) acc[3 * r + c] += (J[r] * J[c] + J[3 + r] * J[3 + c]) + J[6 + r] * J[6 + c];
    }
    const double radius = st->radius;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < r; ++c) A[(size_t)(3 * t + r) * lda + 3 * t + c] = acc[3 * r + c];
      const double d = acc[4 * r];
      A[(size_t)(3 * t + r) * lda + 3 * t + r] = d + lm::lm_diagonal(d, radius);
      A[(size_t)(3 * m) * lda + 3 * t + r] = g[3 * (size_t)t + r];
    }
  } else if (t < m + vg.P) {
    const int p = t - m;
    const int2 rc = vg.pair_rc[p];
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) {
      const int e = vg.pair_edge[k];
      const bool second_is_row = vg.idx[vg.edges[e].y] == rc.x;
      const double* Ja = rec + kRec * (size_t)e + (second_is_row ? 9 : 0);
      const double* Jb = rec + kRec * (size_t)e + (second_is_row ? 0 : 9);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * r + c] += (Ja[r] * Jb[c] + Ja[3 + r] * Jb[3 + c]) + Ja[6 + r] * Jb[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) A[(size_t)(3 * rc.x + r) * lda + 3 * rc.y + c] = acc[3 * r + c];
  }
}

// One lane per free view: the candidate xc = x - scale * y, and the blocks' sums of |x - xc|^2 and |xc|^2.
__global__ __launch_bounds__(kThreads) void k_step(int m, const int* __restrict__ free_view, const double* __restrict__ x,
                                                   const double* __restrict__ scale, const double* __restrict__ y,
                                                   double* __restrict__ xc, double* __restrict__ part,
                                                   const NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  double ss = 0.0, nn = 0.0;
  if (t < m) {
    const size_t v3 = 3 * (size_t)free_view[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double xo = x[v3 + k];
      const double xn = xo - y[3 * (size_t)t + k] * scale[3 * (size_t)t + k];
      xc[v3 + k] = xn;
      const double d = xo - xn;
      ss += d * d; nn += xn * xn;
    }
  }
  const double s0 = block_sum<kThreads>(ss, red), s1 = block_sum<kThreads>(nn, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

struct DecideArgs {
  int nbE, nbM, n3_views;   // blocks of k_candidate, blocks of k_step, 3 * num_views
  int capacity_rows, term_parameter, term_function, term_failure;
  double function_tolerance, parameter_tolerance, max_radius;
};

// One workgroup: sums the blocks' partials in block order, then thread 0 runs one pass of TrustRegionMinimizer's loop
// body in Ceres' order: invalid step (a failed factorisation, a non-finite step, a model cost change that is not
// positive), parameter tolerance, function tolerance, rho > 1e-3, radius update.  On acceptance the workgroup copies the
// candidate over the iterate and marks it fresh.
__global__ __launch_bounds__(kThreads) void k_decide(DecideArgs a, const double* __restrict__ part_cand,
                                                     const double* __restrict__ part_step, double* __restrict__ fail_flag,
                                                     double* __restrict__ x, const double* __restrict__ xc,
                                                     double* __restrict__ trace, NlState* __restrict__ st) {
  __shared__ double red[kThreads];
  __shared__ int flags[2];
  if (threadIdx.x == 0) { flags[0] = st->done; flags[1] = 0; }
  __syncthreads();
  if (flags[0]) return;
  double sum[4];
  for (int c = 0; c < 2; ++c) sum[c] = block_sum_column<kThreads>(part_cand, a.nbE, 2, c, red);
  for (int c = 0; c < 2; ++c) sum[2 + c] = block_sum_column<kThreads>(part_step, a.nbM, 2, c, red);
  if (threadIdx.x == 0) {
    const double failed = *fail_flag;
    *fail_flag = 0.0;
    st->iterations += 1;
    const double model = sum[1], step_sq = sum[2];
    const bool ok = failed == 0.0 && isfinite(step_sq) && isfinite(model) && model > 0.0;
    if (!ok) {
      st->invalid += 1;
      if (!lm::invalid_step(*st)) {
        st->done = 1; st->term = a.term_failure;
      } else {
        trace_row(trace, a.capacity_rows, st, st->cost, st->gmax, 0.0, st->radius, 0);
      }
    } else {
      lm::valid_step(*st);
      double cand = 0.5 * sum[0];
      if (!isfinite(cand)) cand = DBL_MAX;
      const double step_norm = sqrt(step_sq);
      const double change = st->cost - cand;
      if (lm::parameter_rule(step_norm, st->x_norm, a.parameter_tolerance)) {
        trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        st->done = 1; st->term = a.term_parameter;
      } else if (lm::function_rule(st->cost, cand, a.function_tolerance)) {
        trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        st->done = 1; st->term = a.term_function;
      } else {
        const double rho = change / model;
        if (lm::step_accepted(rho)) {
          st->cost = cand;
          st->x_norm = sqrt(sum[3]);
          lm::accept(*st, rho, a.max_radius);
          st->successful += 1; st->fresh = 1;
          trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 1);   // k_post: the new gradient
          flags[1] = 1;
        } else {
          lm::shrink(*st); st->unsuccessful += 1;
          trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        }
      }
    }
  }
  __syncthreads();
  if (flags[1])
    for (int k = threadIdx.x; k < a.n3_views; k += kThreads) x[k] = xc[k];
}

// LM iterations enqueued between two reads of the state: THEIA_HIP_LM_CHUNK, within 1 .. kMaxChunk
inline int lm_chunk_size() {
  const char* chunk_env = getenv("THEIA_HIP_LM_CHUNK");
  return std::max(1, std::min(chunk_env ? atoi(chunk_env) : kDefaultChunk, kMaxChunk));
}

inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }
inline bool nonnegative_finite(double v) { return v >= 0.0 && std::isfinite(v); }

}  // namespace
}  // namespace thip
