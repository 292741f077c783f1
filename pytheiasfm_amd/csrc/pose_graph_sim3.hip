// pose_graph_sim3.hip -- Sim(3) pose-graph optimisation of camera poses: a Ceres Levenberg-Marquardt solve over one
// Sim3ReconAlignErrorTerm (sfm/transformation/pose_graph_sim3_error.h:46-103) per edge, every node on Sim3Manifold
// (align_reconstructions_pose_graph_optim.cc:39-81), nodes optionally held (SetParameterBlockConstant): the problem
// AlignOverlapReconstructionsWithPointsAndPosesRobust (align_reconstructions.h:61-68) declares and the reference never
// defines.  theia_hip_pose_graph_sim3 and the test-only theia_hip_selftest_sim3_pose_graph_term.  The per-edge arithmetic
// is pose_graph_sim3_device.h over sim3_device.h; the step rules are lm_rules.h (the fourteenth loop on them).  This file
// must be compiled without FMA contraction (build.sh's default).  DESIGN.md 3.6x.
//
// The loop is Ceres 2.2's TrustRegionMinimizer + LevenbergMarquardtStrategy on the dense normal equations of order 7m
// (m = the free nodes that have an edge), a sibling of graph_lm.h's loop over 3-vector nodes, on the same shared headers.
// Sim3Manifold's PlusJacobian is the identity, so the solver's Jacobian is the term's.  An edge's record is 56 doubles,
// weighted residual [7] | weighted J_i [7][7], WITHOUT the Jacobi scaling: J_j = -J_i, so the two ends differ by their
// scales only, which are applied where the record is read.
//   k_pg_linearise     one lane per edge: the record at x; the blocks' sums of |residual|^2
//   k_pg_column_norms  first linearisation only, one wavefront per free node over its incident edges: scale = 1 / (1 + |column|)
//   k_pg_gradient      one wavefront per free node over its incident edges: J' r, the scaled right-hand side; max |J' r| per block
//   k_pg_post          one workgroup: gradient max norm, the trace row, then cap / gradient tolerance / radius floor
//   k_pg_assemble      one wavefront per owner, lanes over the 49 entries, edges in edge order: a free node's diagonal block with
//                      the LM diagonal and its part of the right-hand-side row; an unordered pair's off-diagonal block
//   dense_cholesky_factor + dense_cholesky_back_substitute (DenseSpd), device fail flag
//   k_pg_step          one lane per free node: candidate = Plus(x, -scale y) with the clamp; |candidate - x|^2 and |candidate|^2
//                      in the ambient vector per block; a non-finite step or a logarithm outside Sophus' range: NaN (invalid step)
//   k_pg_candidate     one lane per edge: the candidate's |residual|^2 (the linearisation's residual code) and the model cost
//                      change -m . (r + m / 2), m = J_i (delta_i - delta_j)
//   k_pg_decide        one workgroup: Ceres' rules in Ceres' order; copies the candidate over the iterate on acceptance; `done`
// Every kernel returns at once while `done` is set; the host enqueues iterations in chunks (device_util.h run_until_done).
//
// Determinism: no atomics of this file's own (the factorisation's fail flag is only compared with zero).  Every sum has one
// owner and a fixed order: two calls on one input give the same bytes.
#include "pose_graph_sim3_device.h"
#include "dense_cholesky.h"
#include "lm_rules.h"
#include "view_graph_device.h"

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
static_assert(kThreads == 64 * kViewsPerBlock, "one wavefront per owner, kViewsPerBlock owners per workgroup");
constexpr int kRec = 56;            // doubles per edge record: weighted residual [7] | weighted J_i [7][7]
constexpr int kDefaultChunk = 4;    // LM iterations enqueued between two reads of the state
constexpr int kMaxChunk = 64;

struct PgState {
  int done, term, iterations, successful, unsuccessful, invalid;
  int invalid_steps;     // consecutive invalid steps
  int step_successful;   // the last step was accepted (the gradient rule applies after successful steps only)
  int fresh;             // the iterate changed: k_pg_linearise / k_pg_gradient run, k_pg_post takes the new gradient
  int trace_rows, pad0, pad1;
  double cost, initial_cost, gmax, x_norm, radius, decrease_factor;   // (with the two ints above: the state of lm_rules.h)
};

struct PgEdges {   // the edges as the per-edge kernels read them
  int E;
  const int2* edges;
  const int* idx;
  const double* z;   // [E][7] log(Sji)
  const double* W;   // [E][49] or null
};

__device__ __forceinline__ void load7(const double* __restrict__ p, double* v) {
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = p[k];
}

// One lane per edge: the record at x and the blocks' sums of |W r|^2.  An edge between two held nodes is not in the problem.
__global__ __launch_bounds__(kThreads) void k_pg_linearise(PgEdges g, const double* __restrict__ x, double* __restrict__ rec,
                                                           double* __restrict__ part_cost, const PgState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done || !st->fresh) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0;
  if (e < g.E) {
    const int2 ij = g.edges[e];
    if (g.idx[ij.x] >= 0 || g.idx[ij.y] >= 0) {
      double xi[7], xj[7], z[7], res[7];
      load7(x + 7 * (size_t)ij.x, xi);
      load7(x + 7 * (size_t)ij.y, xj);
      load7(g.z + 7 * (size_t)e, z);
      double* o = rec + kRec * (size_t)e;
      sim3::pose_graph_term(xi, xj, z, g.W ? g.W + 49 * (size_t)e : nullptr, res, o + 7);
#pragma unroll
      for (int k = 0; k < 7; ++k) { o[k] = res[k]; rho += res[k] * res[k]; }
    }
  }
  const double s = block_sum<kThreads>(rho, red);
  if (threadIdx.x == 0) part_cost[blockIdx.x] = s;
}

// One wavefront per free node: the squared norms of its seven columns over its incident edges (lane l takes edges l, l + 64,
// .. in order, then the butterfly); scale = 1 / (1 + |column|).  J_j = -J_i: the sign does not enter.
__global__ __launch_bounds__(kThreads) void k_pg_column_norms(ViewGraphLists vg, const double* __restrict__ rec,
                                                              double* __restrict__ scale) {
  const int v = blockIdx.x * kViewsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= vg.m) return;   // wave-uniform
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for_each_incident_edge(vg, v, lane, [&](int e, bool) {
    const double* J = rec + kRec * (size_t)e + 7;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int c = 0; c < 7; ++c) s[c] += J[7 * k + c] * J[7 * k + c];
  });
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const double t = wave_sum_butterfly(s[c]);
    if (lane == 0) scale[7 * (size_t)v + c] = lm::jacobi_scale(t);
  }
}

// One wavefront per free node: J' r over its incident edges (+J_i at the edge's first node, -J_i at its second); g = the
// scaled right-hand side; part_g[block] = max |J' r| over the workgroup's nodes (the gradient of the unscaled problem).
__global__ __launch_bounds__(kThreads) void k_pg_gradient(ViewGraphLists vg, const double* __restrict__ rec,
                                                          const double* __restrict__ scale, double* __restrict__ g,
                                                          double* __restrict__ part_g, const PgState* __restrict__ st) {
  __shared__ double red[kViewsPerBlock];
  if (st->done || !st->fresh) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.x * kViewsPerBlock + wv;
  double gm = 0.0;
  if (v < vg.m) {   // wave-uniform
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_each_incident_edge(vg, v, lane, [&](int e, bool second) {
      const double* R = rec + kRec * (size_t)e;
      const double* J = R + 7;
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) t += J[7 * k + c] * R[k];
        s[c] += second ? -t : t;
      }
    });
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const double t = wave_sum_butterfly(s[c]);
      if (lane == 0) g[7 * (size_t)v + c] = t * scale[7 * (size_t)v + c];
      gm = fmax(gm, fabs(t));
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

__device__ __forceinline__ void trace_row(double* trace, int capacity_rows, PgState* st, double cost, double gmax,
                                          double step, double radius, int accepted) {
  if (st->trace_rows < capacity_rows) {
    double* t = trace + 5 * (size_t)st->trace_rows;
    t[0] = cost; t[1] = gmax; t[2] = step; t[3] = radius; t[4] = (double)accepted;
  }
  st->trace_rows += 1;
}

// One workgroup, after every k_pg_decide and once at the start (init = 1).  When the iterate is fresh: the gradient max norm
// of the new linearisation (at the start also the cost, |x| and trace row 0).  Then the rules that end the loop between two
// iterations, in Ceres' order: at the start the gradient tolerance, then the cap; afterwards the cap, the gradient tolerance
// (after a successful step only), the radius floor.
__global__ __launch_bounds__(kThreads) void k_pg_post(int init, int m, const int* __restrict__ free_view,
                                                      const double* __restrict__ x, const double* __restrict__ part_cost, int nbE,
                                                      const double* __restrict__ part_g, int nbV, int max_iterations,
                                                      double gradient_tolerance, double* __restrict__ trace, int capacity_rows,
                                                      PgState* __restrict__ st) {
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
        const double* w = x + 7 * (size_t)free_view[k];
#pragma unroll
        for (int c = 0; c < 7; ++c) q += w[c] * w[c];
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
  const bool grad = lm::gradient_rule(*st, st->gmax, gradient_tolerance);
  const bool cap = st->iterations >= max_iterations;
  if (init && grad) { st->done = 1; st->term = THEIA_SIM3_TERM_GRADIENT_TOLERANCE; }
  else if (cap) { st->done = 1; st->term = THEIA_SIM3_TERM_MAX_ITERATIONS; }
  else if (grad) { st->done = 1; st->term = THEIA_SIM3_TERM_GRADIENT_TOLERANCE; }
  else if (lm::radius_floor(*st)) { st->done = 1; st->term = THEIA_SIM3_TERM_MIN_RADIUS; }
}

// The lower triangle of Js'Js + D into the cleared array (row-major, leading dimension lda), Js = J diag(scale),
// D = clamp(diag(Js'Js), 1e-6, 1e32) / radius, and g into row 7m, the factorisation's right-hand-side row.  One wavefront
// per owner; lane l < 49 owns entry (l / 7, l % 7) of the owner's block and adds the owner's edges in edge order:
//   owner t < m     : free node t -- its diagonal block, sum of Js'Js over its incident edges; lanes 49 .. 55 copy g
//   owner t = m + p : pair p = (a > b) -- block (a, b) = -sum of (J S_a)'(J S_b) over the pair's edges (J_j = -J_i)
__global__ __launch_bounds__(kThreads) void k_pg_assemble(ViewGraphLists vg, int lda, const double* __restrict__ rec,
                                                          const double* __restrict__ scale, const double* __restrict__ g,
                                                          double* __restrict__ A, const PgState* __restrict__ st) {
  if (st->done) return;
  const int t = blockIdx.x * kViewsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63, m = vg.m;
  if (t >= m + vg.P) return;   // wave-uniform
  const int r = lane / 7, c = lane % 7;
  if (t < m) {
    if (lane < 49) {
      if (c > r) return;
      const double sr = scale[7 * (size_t)t + r], sc = scale[7 * (size_t)t + c];
      double acc = 0.0;
      for (int k = vg.inc_off[t]; k < vg.inc_off[t + 1]; ++k) {
        const double* J = rec + kRec * (size_t)(vg.inc[k] >> 1) + 7;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 7; ++q) s += (J[7 * q + r] * sr) * (J[7 * q + c] * sc);
        acc += s;
      }
      if (r == c) acc += lm::lm_diagonal(acc, st->radius);
      A[(size_t)(7 * t + r) * lda + 7 * t + c] = acc;
    } else if (lane < 56) {
      const int q = lane - 49;
      A[(size_t)(7 * m) * lda + 7 * t + q] = g[7 * (size_t)t + q];
    }
  } else if (lane < 49) {
    const int p = t - m;
    const int2 rc = vg.pair_rc[p];
    const double sr = scale[7 * (size_t)rc.x + r], sc = scale[7 * (size_t)rc.y + c];
    double acc = 0.0;
    for (int k = vg.pair_off[p]; k < vg.pair_off[p + 1]; ++k) {
      const double* J = rec + kRec * (size_t)vg.pair_edge[k] + 7;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 7; ++q) s += (J[7 * q + r] * sr) * (J[7 * q + c] * sc);
      acc -= s;
    }
    A[(size_t)(7 * rc.x + r) * lda + 7 * rc.y + c] = acc;
  }
}

// One lane per free node: the candidate Plus(x, delta), delta = -scale y, and the blocks' sums of |candidate - x|^2 and
// |candidate|^2 in the ambient 7-vector.  A non-finite delta or a logarithm that is not defined leaves NaN in the first sum:
// k_pg_decide then counts an invalid step.
__global__ __launch_bounds__(kThreads) void k_pg_step(int m, const int* __restrict__ free_view, const double* __restrict__ x,
                                                      const double* __restrict__ scale, const double* __restrict__ y,
                                                      double* __restrict__ xc, double* __restrict__ part,
                                                      const PgState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  double ss = 0.0, nn = 0.0;
  if (t < m) {
    const size_t v7 = 7 * (size_t)free_view[t];
    double xo[7], d[7], xn[7];
    bool ok = true;
    load7(x + v7, xo);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      d[k] = -(y[7 * (size_t)t + k] * scale[7 * (size_t)t + k]);
      ok = ok && isfinite(d[k]);
    }
    if (ok) ok = sim3::pose_graph_plus(xo, d, xn);
    if (ok) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        xc[v7 + k] = xn[k];
        const double q = xn[k] - xo[k];
        ss += q * q; nn += xn[k] * xn[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 7; ++k) xc[v7 + k] = xo[k];
      ss = NAN;
    }
  }
  const double s0 = block_sum<kThreads>(ss, red), s1 = block_sum<kThreads>(nn, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

// One lane per edge: |W r|^2 at the candidate, and the model cost change -m . (r + m / 2) with m = J_i (delta_i - delta_j) from
// the record (delta = -scale y, zero for a held node).
__global__ __launch_bounds__(kThreads) void k_pg_candidate(PgEdges g, const double* __restrict__ xc, const double* __restrict__ rec,
                                                           const double* __restrict__ y, const double* __restrict__ scale,
                                                           double* __restrict__ part, const PgState* __restrict__ st) {
  __shared__ double red[kThreads];
  if (st->done) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double rho = 0.0, model = 0.0;
  if (e < g.E) {
    const int2 ij = g.edges[e];
    const int a = g.idx[ij.x], c = g.idx[ij.y];
    if (a >= 0 || c >= 0) {
      double xi[7], xj[7], z[7], res[7], d[7];
      load7(xc + 7 * (size_t)ij.x, xi);
      load7(xc + 7 * (size_t)ij.y, xj);
      load7(g.z + 7 * (size_t)e, z);
      sim3::pose_graph_term(xi, xj, z, g.W ? g.W + 49 * (size_t)e : nullptr, res, nullptr);
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        rho += res[k] * res[k];
        const double di = a >= 0 ? -(y[7 * (size_t)a + k] * scale[7 * (size_t)a + k]) : 0.0;
        const double dj = c >= 0 ? -(y[7 * (size_t)c + k] * scale[7 * (size_t)c + k]) : 0.0;
        d[k] = di - dj;
      }
      const double* R = rec + kRec * (size_t)e;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        double mr = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) mr += R[7 + 7 * r + k] * d[k];
        s += mr * (R[r] + mr / 2.0);
      }
      model = -s;
    }
  }
  const double s0 = block_sum<kThreads>(rho, red), s1 = block_sum<kThreads>(model, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s0; part[2 * blockIdx.x + 1] = s1; }
}

struct DecideArgs {
  int nbE, nbM, n7_nodes;   // blocks of k_pg_candidate, blocks of k_pg_step, 7 * num_nodes
  int capacity_rows;
  double function_tolerance, parameter_tolerance, max_radius;
};

// One workgroup: sums the blocks' partials in block order, then thread 0 runs one pass of TrustRegionMinimizer's loop body in
// Ceres' order: invalid step (a failed factorisation, a non-finite step, a Plus outside Sophus' range, a model cost change
// that is not positive), parameter tolerance, function tolerance, rho > 1e-3, radius update.  On acceptance the workgroup
// copies the candidate over the iterate and marks it fresh.
__global__ __launch_bounds__(kThreads) void k_pg_decide(DecideArgs a, const double* __restrict__ part_cand,
                                                        const double* __restrict__ part_step, double* __restrict__ fail_flag,
                                                        double* __restrict__ x, const double* __restrict__ xc,
                                                        double* __restrict__ trace, PgState* __restrict__ st) {
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
        st->done = 1; st->term = THEIA_SIM3_TERM_FAILURE;
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
        st->done = 1; st->term = THEIA_SIM3_TERM_PARAMETER_TOLERANCE;
      } else if (lm::function_rule(st->cost, cand, a.function_tolerance)) {
        trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 0);
        st->done = 1; st->term = THEIA_SIM3_TERM_FUNCTION_TOLERANCE;
      } else {
        const double rho = change / model;
        if (lm::step_accepted(rho)) {
          st->cost = cand;
          st->x_norm = sqrt(sum[3]);
          lm::accept(*st, rho, a.max_radius);
          st->successful += 1; st->fresh = 1;
          trace_row(trace, a.capacity_rows, st, cand, st->gmax, step_norm, st->radius, 1);   // k_pg_post: the new gradient
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
    for (int k = threadIdx.x; k < a.n7_nodes; k += kThreads) x[k] = xc[k];
}

// Self-check entry: one lane per edge, the linearisation's code on caller-supplied vectors.
__global__ __launch_bounds__(kThreads) void k_pg_selftest_term(int count, const double* __restrict__ x_i,
                                                               const double* __restrict__ x_j, const double* __restrict__ meas,
                                                               const double* __restrict__ W, double* __restrict__ res_out,
                                                               double* __restrict__ jac_out) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= count) return;
  double xi[7], xj[7], z[7], res[7];
  load7(x_i + 7 * (size_t)e, xi);
  load7(x_j + 7 * (size_t)e, xj);
  load7(meas + 7 * (size_t)e, z);
  double* J = jac_out + 49 * (size_t)e;
  if (!sim3::pose_graph_term(xi, xj, z, W ? W + 49 * (size_t)e : nullptr, res, J))
    for (int k = 0; k < 49; ++k) J[k] = NAN;
#pragma unroll
  for (int k = 0; k < 7; ++k) res_out[7 * (size_t)e + k] = res[k];
}

// LM iterations enqueued between two reads of the state: THEIA_HIP_LM_CHUNK, within 1 .. kMaxChunk
inline int lm_chunk_size() {
  const char* chunk_env = getenv("THEIA_HIP_LM_CHUNK");
  return std::max(1, std::min(chunk_env ? atoi(chunk_env) : kDefaultChunk, kMaxChunk));
}
inline bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }
inline bool nonnegative_finite(double v) { return v >= 0.0 && std::isfinite(v); }
inline bool all_finite(const double* p, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(p[k])) return false;
  return true;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_pose_graph_sim3(int32_t num_nodes, double* nodes, const uint8_t* fixed, int32_t num_edges,
                                         const int32_t* edges, const double* measurements, const double* sqrt_information,
                                         const theia_pose_graph_sim3_options* options, theia_pose_graph_sim3_summary* summary,
                                         double* trace_out, int32_t trace_capacity) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_nodes, E = num_edges;
  // ---- refusals, before the device is touched and with nothing written
  if (!summary) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null summary");
  theia_pose_graph_sim3_options o{50, 0, 1e-6, 1e-10, 1e-8, 1e4, 1e16};
  if (options) o = *options;
  if (n < 1 || !nodes) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no nodes, or null nodes");
  if (E < 1 || !edges || !measurements) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative Sim(3) constraints");
  if (trace_capacity < 0 || (trace_capacity > 0 && !trace_out)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad trace buffer");
  if (o.max_num_iterations < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations must be >= 0");
  if (!nonnegative_finite(o.function_tolerance) || !nonnegative_finite(o.gradient_tolerance) ||
      !nonnegative_finite(o.parameter_tolerance))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the tolerances must be finite and not negative");
  if (!positive_finite(o.initial_trust_region_radius) || !positive_finite(o.max_trust_region_radius))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the trust-region radii must be positive and finite");
  std::vector<int> root;
  if (int bad = view_graph_components(n, E, edges, &root)) return bad;
  std::vector<uint8_t> out(n, 1);   // the nodes that take no columns: held, or without an edge
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i == j)   // Ceres refuses a residual block that names one parameter block twice
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d joins node %d to itself", e, i);
    out[i] = out[j] = 0;
  }
  if (!all_finite(nodes, 7 * (size_t)n)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a node is not finite");
  if (!all_finite(measurements, 7 * (size_t)E)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a measurement is not finite");
  if (sqrt_information && !all_finite(sqrt_information, 49 * (size_t)E))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a sqrt_information entry is not finite");
  for (int v = 0; v < n && fixed; ++v) if (fixed[v]) out[v] = 1;
  ViewGraphPlan g;
  fill_view_graph_lists(n, out, E, edges, &g);
  const int m = g.m;
  theia_pose_graph_sim3_summary sm{};
  sm.num_nodes_in_problem = m;
  if (m == 0) {   // every node of every edge is held: nothing to solve
    sm.seconds = ms_since(t_start) * 1e-3;
    *summary = sm;
    return 0;
  }
  if ((long long)m * 7 + 1 > INT32_MAX / 2) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d nodes: the dense system does not fit", m);
  const int n7 = 7 * m;

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  hipStream_t st = nullptr;
  const int nbE = grid_of(E, kThreads), nbM = grid_of(m, kThreads), nbV = grid_of(m, kViewsPerBlock);
  const int rows = o.max_num_iterations + 1;
  DenseSpd A;   // row n7: the right-hand side
  DeviceViewGraph dg;
  DevBuf<double> d_x, d_xc, d_z, d_W, d_rec, d_scale, d_g, d_y, d_pc, d_pg, d_pcand, d_pstep, d_trace;
  DevBuf<PgState> d_st;
  // the dense system first: when it does not fit, that is the answer
  if ((rc = A.alloc(n7, 1)) || (rc = d_x.up(nodes, 7 * (size_t)n)) || (rc = d_xc.up(nodes, 7 * (size_t)n)) ||
      (rc = d_z.up(measurements, 7 * (size_t)E)) || (sqrt_information && (rc = d_W.up(sqrt_information, 49 * (size_t)E))) ||
      (rc = dg.up(g, edges, E, n)) || (rc = d_rec.alloc(kRec * (size_t)E)) || (rc = d_scale.alloc(n7)) || (rc = d_g.alloc(n7)) ||
      (rc = d_y.alloc(n7)) || (rc = d_pc.alloc(nbE)) || (rc = d_pg.alloc(nbV)) || (rc = d_pcand.alloc(2 * (size_t)nbE)) ||
      (rc = d_pstep.alloc(2 * (size_t)nbM)) || (rc = d_trace.alloc(5 * (size_t)rows)) || (rc = d_st.alloc(1)))
    return rc;
  const ViewGraphLists& vg = dg.lists;
  const PgEdges pe{E, vg.edges, vg.idx, d_z.p, sqrt_information ? d_W.p : nullptr};

  PgState hs{};
  lm::start(hs); hs.fresh = 1;
  hs.radius = o.initial_trust_region_radius;
  HIP_TRY(hipMemcpy(d_st.p, &hs, sizeof(PgState), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(A.flag(), 0, sizeof(double), st));
  HIP_TRY(hipMemsetAsync(d_rec.p, 0, sizeof(double) * kRec * (size_t)E, st));
  const int* done = &d_st.p->done;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, st));

  auto linearise_and_post = [&](int init) {
    k_pg_linearise<<<nbE, kThreads, 0, st>>>(pe, d_x.p, d_rec.p, d_pc.p, d_st.p);
    if (init) k_pg_column_norms<<<nbV, kThreads, 0, st>>>(vg, d_rec.p, d_scale.p);
    k_pg_gradient<<<nbV, kThreads, 0, st>>>(vg, d_rec.p, d_scale.p, d_g.p, d_pg.p, d_st.p);
    k_pg_post<<<1, kThreads, 0, st>>>(init, m, vg.free_view, d_x.p, d_pc.p, nbE, d_pg.p, nbV, o.max_num_iterations,
                                      o.gradient_tolerance, d_trace.p, rows, d_st.p);
  };
  // ---- the first linearisation and the Jacobi scaling from its columns
  linearise_and_post(1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(&hs, d_st.p, sizeof(PgState), hipMemcpyDeviceToHost));

  // ---- the LM loop
  const DecideArgs da{nbE, nbM, 7 * n, rows, o.function_tolerance, o.parameter_tolerance, o.max_trust_region_radius};
  rc = run_until_done(o.max_num_iterations, lm_chunk_size(), d_st.p, &hs, [&]() {
    if (int bad = A.clear(st)) return bad;
    k_pg_assemble<<<grid_of((size_t)m + g.P, kViewsPerBlock), kThreads, 0, st>>>(vg, A.lda, d_rec.p, d_scale.p, d_g.p, A.A(), d_st.p);
    A.factor(1, st, done);
    A.back_substitute(1, A.rhs_row(0), A.lda, d_y.p, st, done);
    k_pg_step<<<nbM, kThreads, 0, st>>>(m, vg.free_view, d_x.p, d_scale.p, d_y.p, d_xc.p, d_pstep.p, d_st.p);
    k_pg_candidate<<<nbE, kThreads, 0, st>>>(pe, d_xc.p, d_rec.p, d_y.p, d_scale.p, d_pcand.p, d_st.p);
    k_pg_decide<<<1, kThreads, 0, st>>>(da, d_pcand.p, d_pstep.p, A.flag(), d_x.p, d_xc.p, d_trace.p, d_st.p);
    linearise_and_post(0);
    return 0;
  });
  float kernel_ms = 0.f;
  {
    hipError_t r = hipEventRecord(e1, st);
    if (r == hipSuccess) r = hipEventSynchronize(e1);
    if (r == hipSuccess) r = hipEventElapsedTime(&kernel_ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    HIP_TRY(r);
  }
  if (!hs.done) return set_error(THEIA_HIP_ERR_INTERNAL, "the loop ended without a termination");

  // ---- Ceres copies its state back unless the solve failed; held and edgeless nodes keep their bits
  std::vector<double> x, tr;
  if (hs.term != THEIA_SIM3_TERM_FAILURE) {
    x.resize(7 * (size_t)n);
    HIP_TRY(hipMemcpy(x.data(), d_x.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost));
  }
  const int have = std::min(hs.trace_rows, rows);
  sm.trace_size = std::min(have, (int)trace_capacity);
  if (sm.trace_size > 0) {
    tr.resize(5 * (size_t)sm.trace_size);
    HIP_TRY(hipMemcpy(tr.data(), d_trace.p, sizeof(double) * tr.size(), hipMemcpyDeviceToHost));
  }
  if (!x.empty())
    for (int v = 0; v < n; ++v)
      if (g.idx[v] >= 0)
        for (int c = 0; c < 7; ++c) nodes[7 * (size_t)v + c] = x[7 * (size_t)v + c];
  std::copy(tr.begin(), tr.end(), trace_out);
  sm.iterations = hs.iterations;
  sm.num_successful_steps = hs.successful;
  sm.num_unsuccessful_steps = hs.unsuccessful;
  sm.num_invalid_steps = hs.invalid;
  sm.termination = hs.term;
  sm.initial_cost = hs.initial_cost;
  sm.final_cost = hs.cost;
  sm.final_radius = hs.radius;
  sm.final_gradient_max_norm = hs.gmax;
  sm.kernel_ms = kernel_ms;
  sm.seconds = ms_since(t_start) * 1e-3;
  *summary = sm;
  return 0;
}

extern "C" int theia_hip_selftest_sim3_pose_graph_term(int32_t num_edges, const double* x_i, const double* x_j,
                                                       const double* measurements, const double* sqrt_information,
                                                       double* residual_out, double* jacobian_i_out) {
  const int count = num_edges;
  if (count < 1 || count > (1 << 20)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_edges = %d", count);
  if (!x_i || !x_j || !measurements || !residual_out || !jacobian_i_out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  int rc = thip::ensure_device();
  if (rc) return rc;
  DevBuf<double> d_i, d_j, d_z, d_W, d_r, d_J;
  const size_t n7 = 7 * (size_t)count, n49 = 49 * (size_t)count;
  if ((rc = d_i.up(x_i, n7)) || (rc = d_j.up(x_j, n7)) || (rc = d_z.up(measurements, n7)) ||
      (sqrt_information && (rc = d_W.up(sqrt_information, n49))) || (rc = d_r.alloc(n7)) || (rc = d_J.alloc(n49)))
    return rc;
  k_pg_selftest_term<<<grid_of(count, kThreads), kThreads, 0, nullptr>>>(count, d_i.p, d_j.p, d_z.p,
                                                                          sqrt_information ? d_W.p : nullptr, d_r.p, d_J.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(residual_out, d_r.p, sizeof(double) * n7, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(jacobian_i_out, d_J.p, sizeof(double) * n49, hipMemcpyDeviceToHost));
  return 0;
}
