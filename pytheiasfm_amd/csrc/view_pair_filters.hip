// view_pair_filters.hip -- the two view-graph filters of the global pipeline (sfm/global_reconstruction_estimator.cc:126-138,
// steps 4 and 6) on the device:
//   FilterViewPairsFromRelativeTranslation (sfm/filter_view_pairs_from_relative_translation.cc:264-312): Wilson & Snavely's
//     1DSfM test.  The translations are rotated into the global frame, projected on num_iterations random axes, and per axis
//     the views are ordered by a greedy minimum-feedback-arc-set heuristic; a pair whose projections contradict the
//     orderings by more than tolerance * num_iterations in total is removed.
//   FilterViewPairsFromOrientation (sfm/filter_view_pairs_from_orientation.cc:46-103): one loop-rotation residual per pair.
//
// Kernels
//   k_rotate      per pair AngleAxisRotatePoint(-orientation[first], position_2) and the block partials of the sum;
//   k_sq_dev      the block partials of the squared deviations from the mean;  k_reduce3 sums either in block order.
//   k_project     proj[it][e] = t_e . axis_it, and the same value per slot of the adjacency lists (padj[it][k]), so that the
//                 ordering's neighbour walk reads its weights with the stride of the walk.
//                 The dot product is three products and two sums, (t0 a0 + t1 a1) + t2 a2, uncontracted (the file is compiled
//                 with -ffp-contract=off): a host restatement of it is bit-equal given the same rotated translations.
//   k_mfas_order  OrderTranslationsFromProjections (:108-160), one workgroup per iteration.  Per view: the incoming and
//                 outgoing weight, the live in-degree and a 64-bit selection key (0: removed or never named; all-ones high
//                 word and ~view: a source; else the bit pattern of the score (out + 1.0) / (in + 1.0), which orders like
//                 the score because it is positive).  A step takes the largest key, the lowest view on ties: a source with
//                 the lowest index when there is one, else the arg-max of the score -- per lane over its views, per wave on
//                 the DPP network (wave_reduce.h), across waves through 16 slots of LDS.  Then the lanes walk the chosen
//                 view's adjacency, one neighbour each: the neighbour's weight on that side is DECREMENTED as the reference
//                 does, its in-degree drops if the edge came from the chosen view, its key is recomputed (true division).
//                 Pairs are unique, so a neighbour is touched once per step: no atomics.  Two barriers per step.
//                 The per-view state takes 28 bytes.  Up to kMfasLdsMaxViews = THEIA_MFAS_LDS_MAX_VIEWS = 5 632 views it
//                 lives in LDS (154 KiB of the CU's 160 KiB, plus the 192 bytes of the wave slots); beyond that in a
//                 per-iteration global workspace, the same code on global pointers.
//   k_bad_weight  per pair over the iterations in iteration order (:236-259), then removed = weight > tolerance * iterations.
//   k_orientation_filter  AngularDifferenceIsAcceptable (filter_view_pairs_from_orientation.cc:46-63).
//
// Rules where the reference leaves the choice to the iteration order of its hash maps: the lowest view
// index among the sources; the lowest view index among equal scores; a view's initial weights are summed over its pairs in
// pair order; the iterations add into a pair's weight in iteration order.  No atomics anywhere: two runs are bit-identical.
#include "rotation_maps.h"
#include "wave_reduce.h"
#include "device_util.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int theia_hip_rng_rand_gaussian(theia_rng_state* state, double mean, double std_dev, int32_t n, double* out);

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kMfasMaxThreads = 1024;
constexpr int kMfasMaxWaves = kMfasMaxThreads / 64;
constexpr int kMfasLdsMaxViews = THEIA_MFAS_LDS_MAX_VIEWS;   // the switch point: more views than this take the global workspace
constexpr int kMfasStateBytes = 28;                          // key 8, incoming 8, outgoing 8, in-degree 4
constexpr unsigned kSecondBit = 0x80000000u;                 // adjacency entry: the list's owner is the pair's second view
static_assert((size_t)kMfasLdsMaxViews * kMfasStateBytes + 3 * kMfasMaxWaves * 4 <= 160 * 1024, "the CU has 160 KiB of LDS");

// ceres/rotation.h AngleAxisRotatePoint: Rodrigues for theta^2 > DBL_EPSILON, else pt + aa x pt.
__device__ __forceinline__ void angle_axis_rotate_point(const double* aa, const double* pt, double* out) {
  const double theta2 = (aa[0] * aa[0] + aa[1] * aa[1]) + aa[2] * aa[2];
  if (theta2 > DBL_EPSILON) {
    const double theta = sqrt(theta2);
    const double costheta = cos(theta), sintheta = sin(theta);
    const double theta_inverse = 1.0 / theta;
    const double w[3] = {aa[0] * theta_inverse, aa[1] * theta_inverse, aa[2] * theta_inverse};
    const double c[3] = {w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]};
    const double tmp = ((w[0] * pt[0] + w[1] * pt[1]) + w[2] * pt[2]) * (1.0 - costheta);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (pt[k] * costheta + c[k] * sintheta) + w[k] * tmp;
  } else {
    out[0] = pt[0] + (aa[1] * pt[2] - aa[2] * pt[1]);
    out[1] = pt[1] + (aa[2] * pt[0] - aa[0] * pt[2]);
    out[2] = pt[2] + (aa[0] * pt[1] - aa[1] * pt[0]);
  }
}

// RotateRelativeTranslationsToGlobalFrame (:67-84); part[block][3] = the block's sums of the three components.
__global__ __launch_bounds__(kThreads) void k_rotate(int E, const int2* __restrict__ pairs, const double* __restrict__ aa,
                                                     const double* __restrict__ rel, double* __restrict__ rot,
                                                     double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double r[3] = {0.0, 0.0, 0.0};
  if (e < E) {
    const int i = pairs[e].x;
    const double w[3] = {-aa[3 * (size_t)i], -aa[3 * (size_t)i + 1], -aa[3 * (size_t)i + 2]};
    const double t[3] = {rel[3 * (size_t)e], rel[3 * (size_t)e + 1], rel[3 * (size_t)e + 2]};
    angle_axis_rotate_point(w, t, r);
    rot[3 * (size_t)e] = r[0]; rot[3 * (size_t)e + 1] = r[1]; rot[3 * (size_t)e + 2] = r[2];
  }
  const double s0 = block_sum<kThreads>(r[0], red), s1 = block_sum<kThreads>(r[1], red), s2 = block_sum<kThreads>(r[2], red);
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = s0; part[3 * blockIdx.x + 1] = s1; part[3 * blockIdx.x + 2] = s2; }
}

// ComputeMeanVariance's second loop (:190-193): (t - mean)^2 per component.
__global__ __launch_bounds__(kThreads) void k_sq_dev(int E, const double* __restrict__ rot, const double* __restrict__ mean,
                                                     double* __restrict__ part) {
  __shared__ double red[kThreads];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double d[3] = {0.0, 0.0, 0.0};
  if (e < E) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = rot[3 * (size_t)e + k] - mean[k];
      d[k] = v * v;
    }
  }
  const double s0 = block_sum<kThreads>(d[0], red), s1 = block_sum<kThreads>(d[1], red), s2 = block_sum<kThreads>(d[2], red);
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = s0; part[3 * blockIdx.x + 1] = s1; part[3 * blockIdx.x + 2] = s2; }
}

// out[k] = (sum of part[block][k] in block order) / divisor, one workgroup (mean: E, variance: E - 1).
__global__ __launch_bounds__(kThreads) void k_reduce3(int nb, const double* __restrict__ part, double divisor,
                                                      double* __restrict__ out) {
  __shared__ double red[kThreads];
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += kThreads) s += part[3 * (size_t)b + k];
    const double t = block_sum<kThreads>(s, red);
    if (threadIdx.x == 0) out[k] = t / divisor;
  }
}

// ProjectTranslationsOntoAxis (:163-175) for every iteration: thread t < E writes proj[it][t]; thread E + k writes the
// same dot product of the pair behind adjacency slot k to padj[it][k].
__global__ __launch_bounds__(kThreads) void k_project(int E, int iters, const double* __restrict__ rot,
                                                      const double* __restrict__ axes, const int* __restrict__ adj_pair,
                                                      double* __restrict__ proj, double* __restrict__ padj) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= 3 * E) return;
  const bool slot = t >= E;
  const int e = slot ? adj_pair[t - E] : t;
  const double t0 = rot[3 * (size_t)e], t1 = rot[3 * (size_t)e + 1], t2 = rot[3 * (size_t)e + 2];
  double* out = slot ? padj + (t - E) : proj + t;
  const size_t stride = slot ? 2 * (size_t)E : (size_t)E;
  for (int it = 0; it < iters; ++it)
    out[(size_t)it * stride] = (t0 * axes[3 * it] + t1 * axes[3 * it + 1]) + t2 * axes[3 * it + 2];
}

// (key, view) with the largest key and, among equal keys, the lowest view, over the wave; uniform on return.
__device__ __forceinline__ void wave_arg_max(unsigned& hi, unsigned& lo, unsigned& view) {
  const unsigned hm = wave_max_u32(hi);
  const unsigned lm = wave_max_u32(hi == hm ? lo : 0u);
  const unsigned vm = wave_max_u32((hi == hm && lo == lm) ? ~view : 0u);
  hi = hm; lo = lm; view = ~vm;
}

// FindNextViewInOrder's score (:96-97) as a key: positive scores order like their bit patterns.  A score that is not
// positive (a NaN projection) can never be chosen by the reference, which then fails; here such a view keeps the lowest
// non-zero key, so the ordering still ends.
__device__ __forceinline__ unsigned long long score_key(double in_w, double out_w) {
  const double score = (out_w + 1.0) / (in_w + 1.0);
  return score > 0.0 ? (unsigned long long)__double_as_longlong(score) : 1ull;
}
__device__ __forceinline__ unsigned long long source_key(int v) { return 0xFFFFFFFF00000000ull | (unsigned)~v; }

// bytes of one iteration's per-view state in the global workspace (8-byte aligned: the keys come first)
__host__ __device__ inline size_t mfas_state_stride(int N) { return ((size_t)N * kMfasStateBytes + 7) & ~(size_t)7; }

extern __shared__ unsigned long long mfas_lds[];

// One workgroup per iteration.  adj_off / adj_view / padj: the undirected CSR (entry = neighbour, kSecondBit set when the
// list's owner is the pair's second view) and this iteration's projections per slot.  order[it][v]: the step that took
// view v, -1 for a view without pairs.  steps[it][2]: steps that took a source, steps that took the arg-max of the score.
template <bool kLds>
__global__ __launch_bounds__(kMfasMaxThreads) void k_mfas_order(int N, int named, size_t slots,
                                                                const int* __restrict__ adj_off,
                                                                const unsigned* __restrict__ adj_view,
                                                                const double* __restrict__ padj_all, char* __restrict__ ws,
                                                                int* __restrict__ order_all, int* __restrict__ steps) {
  const int it = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  const double* __restrict__ padj = padj_all + (size_t)it * slots;
  int* __restrict__ order = order_all + (size_t)it * N;
  unsigned long long* key;
  double *in_w, *out_w;
  int* indeg;
  unsigned* slot_mem;
  if (kLds) {
    key = mfas_lds;
    in_w = reinterpret_cast<double*>(key + N);
    out_w = in_w + N;
    indeg = reinterpret_cast<int*>(out_w + N);
    slot_mem = reinterpret_cast<unsigned*>(indeg + N);
  } else {
    key = reinterpret_cast<unsigned long long*>(ws + (size_t)it * mfas_state_stride(N));
    in_w = reinterpret_cast<double*>(key + N);
    out_w = in_w + N;
    indeg = reinterpret_cast<int*>(out_w + N);
    slot_mem = reinterpret_cast<unsigned*>(mfas_lds);
  }
  unsigned* s_hi = slot_mem;
  unsigned* s_lo = slot_mem + kMfasMaxWaves;
  unsigned* s_view = slot_mem + 2 * kMfasMaxWaves;

  // the MFAS graph of this iteration (:113-130): a view's weights are summed over its pairs in pair order
  for (int v = tid; v < N; v += T) {
    double wi = 0.0, wo = 0.0;
    int di = 0;
    const int k0 = adj_off[v], k1 = adj_off[v + 1];
    for (int k = k0; k < k1; ++k) {
      const double p = padj[k];
      const bool outgoing = (p > 0.0) != ((adj_view[k] & kSecondBit) != 0u);   // p > 0: first -> second, else second -> first
      if (outgoing) wo += fabs(p); else { wi += fabs(p); ++di; }
    }
    in_w[v] = wi; out_w[v] = wo; indeg[v] = di;
    key[v] = k1 == k0 ? 0ull : (di == 0 ? source_key(v) : score_key(wi, wo));
    if (k1 == k0) order[v] = -1;
  }
  __syncthreads();

  int n_source = 0;
  for (int step = 0; step < named; ++step) {
    // (a) the view to take
    unsigned hi = 0u, lo = 0u, view = 0xFFFFFFFFu;
    for (int v = tid; v < N; v += T) {
      const unsigned long long kv = key[v];
      const unsigned h = (unsigned)(kv >> 32), l = (unsigned)kv;
      if (h > hi || (h == hi && l > lo)) { hi = h; lo = l; view = (unsigned)v; }   // v ascends: ties keep the lowest
    }
    wave_arg_max(hi, lo, view);
    if (lane == 0) { s_hi[wave] = hi; s_lo[wave] = lo; s_view[wave] = view; }
    __syncthreads();
    hi = lane < waves ? s_hi[lane] : 0u;
    lo = lane < waves ? s_lo[lane] : 0u;
    view = lane < waves ? s_view[lane] : 0xFFFFFFFFu;
    wave_arg_max(hi, lo, view);
    if (hi == 0u && lo == 0u) break;   // no live view (cannot happen while step < named); uniform
    const int c = (int)view;
    n_source += hi == 0xFFFFFFFFu ? 1 : 0;
    // (b) remove it (:140-156): every live neighbour loses the pair's weight on its side
    const int k0 = adj_off[c], k1 = adj_off[c + 1];
    for (int k = k0 + tid; k < k1; k += T) {
      const unsigned a = adj_view[k];
      const int u = (int)(a & ~kSecondBit);
      if (key[u] != 0ull) {
        const double p = padj[k];
        const bool outgoing = (p > 0.0) != ((a & kSecondBit) != 0u);   // from c to u
        double wi = in_w[u], wo = out_w[u];
        int di = indeg[u];
        if (outgoing) { wi -= fabs(p); in_w[u] = wi; --di; indeg[u] = di; } else { wo -= fabs(p); out_w[u] = wo; }
        key[u] = di == 0 ? source_key(u) : score_key(wi, wo);
      }
    }
    if (tid == 0) { key[c] = 0ull; order[c] = step; }   // no pair joins c to itself: the walk above never reads key[c]
    __syncthreads();
  }
  if (tid == 0) { steps[2 * it] = n_source; steps[2 * it + 1] = named - n_source; }
}

// The bad-edge weights (:236-259) in iteration order, and the verdict (:296-305).
__global__ __launch_bounds__(kThreads) void k_bad_weight(int E, int N, int iters, const int2* __restrict__ pairs,
                                                         const double* __restrict__ proj, const int* __restrict__ order,
                                                         double threshold, double* __restrict__ weight,
                                                         uint8_t* __restrict__ removed) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const int2 ij = pairs[e];
  double w = 0.0;
  for (int it = 0; it < iters; ++it) {
    const int diff = order[(size_t)it * N + ij.y] - order[(size_t)it * N + ij.x];
    const double p = proj[(size_t)it * E + e];
    if ((diff < 0 && p > 0.0) || (diff > 0 && p < 0.0)) w += fabs(p);
  }
  weight[e] = w;
  removed[e] = w > threshold ? 1 : 0;
}

// AngularDifferenceIsAcceptable (filter_view_pairs_from_orientation.cc:46-63): a pair stays when
// |MultiplyRotations(-rotation_2, MultiplyRotations(r_second, -r_first))|^2 <= sq_max; a pair naming a view without an
// orientation is removed (:73-82).
__global__ __launch_bounds__(kThreads) void k_orientation_filter(int E, const int2* __restrict__ pairs,
                                                                 const double* __restrict__ aa,
                                                                 const uint8_t* __restrict__ has, const double* __restrict__ rel,
                                                                 double sq_max, uint8_t* __restrict__ removed) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const int2 ij = pairs[e];
  if (has && (!has[ij.x] || !has[ij.y])) { removed[e] = 1; return; }
  const double nr1[3] = {-aa[3 * (size_t)ij.x], -aa[3 * (size_t)ij.x + 1], -aa[3 * (size_t)ij.x + 2]};
  const double r2[3] = {aa[3 * (size_t)ij.y], aa[3 * (size_t)ij.y + 1], aa[3 * (size_t)ij.y + 2]};
  const double nrel[3] = {-rel[3 * (size_t)e], -rel[3 * (size_t)e + 1], -rel[3 * (size_t)e + 2]};
  double composed[3], loop[3];
  multiply_rotations(r2, nr1, composed);
  multiply_rotations(nrel, composed, loop);
  const double sq = (loop[0] * loop[0] + loop[1] * loop[1]) + loop[2] * loop[2];
  removed[e] = sq <= sq_max ? 0 : 1;
}

// What both filters refuse in their pair list: a view out of range, a self-pair, an unordered pair named twice.
int check_pairs(int n_views, int n_pairs, const int32_t* pairs) {
  std::vector<uint64_t> keys((size_t)n_pairs);
  for (int e = 0; e < n_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    if (i < 0 || i >= n_views || j < 0 || j >= n_views)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %d names a view out of range", e);
    if (i == j) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %d names view %d twice", e, i);
    keys[e] = ((uint64_t)std::min(i, j) << 32) | (uint64_t)std::max(i, j);
  }
  std::sort(keys.begin(), keys.end());
  for (int e = 1; e < n_pairs; ++e)
    if (keys[e] == keys[e - 1])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the pair (%d, %d) is listed twice", (int)(keys[e] >> 32),
                       (int)(keys[e] & 0xFFFFFFFFu));
  return 0;
}

thread_local theia_translation_filter_stats g_stats{};

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_filter_view_pairs_from_relative_translation(
    int32_t n_views, int32_t n_pairs, const int32_t* pairs, const double* orientations, const double* position_2,
    const theia_translation_filter_options* opt, theia_rng_state* rng, const double* axes_in, uint8_t* removed,
    double* bad_weight, int32_t* order, double* axes_out, double* rotated) {
  const auto t_start = std::chrono::steady_clock::now();
  const int N = n_views, E = n_pairs;
  const int iters = opt ? opt->num_iterations : 48;
  const double tolerance = opt ? opt->translation_projection_tolerance : 0.08;
  if (N < 0 || E < 0 || !removed || (E > 0 && (!pairs || !orientations || !position_2)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument or negative count");
  if (iters <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_iterations must be positive");
  if (!(tolerance >= 0.0)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the tolerance is negative or NaN");
  if (!rng && !axes_in) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "neither a generator nor axes");
  if (rng && (rng->pos < 0 || rng->pos > 624)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "generator: pos outside [0, 624]");
  int rc = check_pairs(N, E, pairs);
  if (rc) return rc;
  theia_translation_filter_stats stats{};

  if (E < 2) {
    // the variance divides by n_pairs - 1 (:194): the axes are NaN, no comparison of :249-250 holds and nothing is removed.
    // The reference still takes its draws, whose length does not depend on their parameters.
    std::vector<double> draws(3 * (size_t)iters);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!axes_in && (rc = theia_hip_rng_rand_gaussian(rng, nan, nan, 3 * iters, draws.data()))) return rc;
    for (int e = 0; e < E; ++e) { removed[e] = 0; if (bad_weight) bad_weight[e] = 0.0; }
    g_stats = stats;
    return 0;
  }

  // one undirected CSR in pair order: entry = neighbour | kSecondBit when the owner is the pair's second view
  std::vector<int> adj_off((size_t)N + 1, 0), adj_pair(2 * (size_t)E);
  std::vector<unsigned> adj_view(2 * (size_t)E);
  for (int e = 0; e < E; ++e) { ++adj_off[pairs[2 * e] + 1]; ++adj_off[pairs[2 * e + 1] + 1]; }
  int named = 0, max_deg = 0;
  for (int v = 0; v < N; ++v) {
    named += adj_off[v + 1] > 0 ? 1 : 0;
    max_deg = std::max(max_deg, adj_off[v + 1]);
    adj_off[v + 1] += adj_off[v];
  }
  {
    std::vector<int> fill(adj_off.begin(), adj_off.end() - 1);
    for (int e = 0; e < E; ++e) {
      const int i = pairs[2 * e], j = pairs[2 * e + 1];
      adj_view[fill[i]] = (unsigned)j; adj_pair[fill[i]++] = e;
      adj_view[fill[j]] = (unsigned)i | kSecondBit; adj_pair[fill[j]++] = e;
    }
  }
  const bool lds = N <= kMfasLdsMaxViews;
  const size_t slots = 2 * (size_t)E;
  const int nbE = grid_of(E, kThreads);

  if ((rc = thip::ensure_device())) return rc;
  DevBuf<int2> d_pairs;
  DevBuf<double> d_aa, d_rel, d_rot, d_part, d_stat, d_axes, d_proj, d_padj, d_weight;
  DevBuf<int> d_adj_off, d_adj_pair, d_order, d_steps;
  DevBuf<unsigned> d_adj_view;
  DevBuf<char> d_ws;
  DevBuf<uint8_t> d_removed;
  if ((rc = d_pairs.up(pairs, E)) || (rc = d_aa.up(orientations, 3 * (size_t)N)) || (rc = d_rel.up(position_2, 3 * (size_t)E)) ||
      (rc = d_adj_off.up(adj_off.data(), adj_off.size())) || (rc = d_adj_pair.up(adj_pair.data(), slots)) ||
      (rc = d_adj_view.up(adj_view.data(), slots)) || (rc = d_rot.alloc(3 * (size_t)E)) || (rc = d_part.alloc(3 * (size_t)nbE)) ||
      (rc = d_stat.alloc(6)) || (rc = d_axes.alloc(3 * (size_t)iters)) || (rc = d_proj.alloc((size_t)iters * E)) ||
      (rc = d_padj.alloc((size_t)iters * slots)) || (rc = d_order.alloc((size_t)iters * N)) || (rc = d_steps.alloc(2 * (size_t)iters)) ||
      (rc = d_ws.alloc(lds ? 1 : (size_t)iters * mfas_state_stride(N))) || (rc = d_weight.alloc(E)) || (rc = d_removed.alloc(E)))
    return rc;
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamSynchronize(st));
  stats.setup_ms = ms_since(t_start);

  // ---- rotate, mean and variance (:67-84, :178-195), axes (:212-217), projections
  const auto t_rotate = std::chrono::steady_clock::now();
  k_rotate<<<nbE, kThreads, 0, st>>>(E, d_pairs.p, d_aa.p, d_rel.p, d_rot.p, d_part.p);
  k_reduce3<<<1, kThreads, 0, st>>>(nbE, d_part.p, (double)E, d_stat.p);
  k_sq_dev<<<nbE, kThreads, 0, st>>>(E, d_rot.p, d_stat.p, d_part.p);
  k_reduce3<<<1, kThreads, 0, st>>>(nbE, d_part.p, (double)(E - 1), d_stat.p + 3);
  HIP_TRY(hipGetLastError());
  std::vector<double> axes(3 * (size_t)iters);
  if (axes_in) {
    std::memcpy(axes.data(), axes_in, sizeof(double) * axes.size());
  } else {
    double mv[6];
    HIP_TRY(hipMemcpy(mv, d_stat.p, sizeof(mv), hipMemcpyDeviceToHost));
    theia_rng_state local = *rng;   // the caller's state moves only once the call can no longer be refused
    for (int it = 0; it < iters; ++it) {
      double v[3];
      // RandGaussian(mean[k], variance[k]): the reference hands the variance over as the standard deviation (:213-215)
      for (int k = 0; k < 3; ++k)
        if ((rc = theia_hip_rng_rand_gaussian(&local, mv[k], mv[3 + k], 1, &v[k]))) return rc;
      const double z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];   // Eigen's normalized(): v / sqrt(|v|^2) when |v|^2 > 0
      const double nrm = std::sqrt(z);
      for (int k = 0; k < 3; ++k) axes[3 * (size_t)it + k] = z > 0.0 ? v[k] / nrm : v[k];
    }
    *rng = local;
  }
  HIP_TRY(hipMemcpyAsync(d_axes.p, axes.data(), sizeof(double) * axes.size(), hipMemcpyHostToDevice, st));
  k_project<<<grid_of(3 * (size_t)E, kThreads), kThreads, 0, st>>>(E, iters, d_rot.p, d_axes.p, d_adj_pair.p, d_proj.p, d_padj.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  stats.rotate_project_ms = ms_since(t_rotate);

  // ---- the orderings
  const auto t_order = std::chrono::steady_clock::now();
  HIP_TRY(hipMemsetAsync(d_order.p, 0xFF, sizeof(int) * (size_t)iters * N, st));
  const int threads = std::min(kMfasMaxThreads, std::max(64, (std::max(N, max_deg) + 63) / 64 * 64));
  const size_t slot_bytes = 3 * kMfasMaxWaves * sizeof(unsigned);
  if (lds) {
    const size_t bytes = (size_t)N * kMfasStateBytes + slot_bytes;
    static bool raised = false;   // one attribute per process: the kernel may take the CU's whole LDS
    if (!raised) {
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mfas_order<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)((size_t)kMfasLdsMaxViews * kMfasStateBytes + slot_bytes)));
      raised = true;
    }
    k_mfas_order<true><<<iters, threads, bytes, st>>>(N, named, slots, d_adj_off.p, d_adj_view.p, d_padj.p, nullptr, d_order.p,
                                                      d_steps.p);
  } else {
    k_mfas_order<false><<<iters, threads, slot_bytes, st>>>(N, named, slots, d_adj_off.p, d_adj_view.p, d_padj.p, d_ws.p,
                                                            d_order.p, d_steps.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  stats.order_ms = ms_since(t_order);

  // ---- weights and verdicts
  const auto t_weight = std::chrono::steady_clock::now();
  k_bad_weight<<<nbE, kThreads, 0, st>>>(E, N, iters, d_pairs.p, d_proj.p, d_order.p, tolerance * iters, d_weight.p, d_removed.p);
  HIP_TRY(hipGetLastError());
  std::vector<int> steps(2 * (size_t)iters);
  HIP_TRY(hipMemcpy(removed, d_removed.p, (size_t)E, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(steps.data(), d_steps.p, sizeof(int) * steps.size(), hipMemcpyDeviceToHost));
  if (bad_weight) HIP_TRY(hipMemcpy(bad_weight, d_weight.p, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost));
  if (order) HIP_TRY(hipMemcpy(order, d_order.p, sizeof(int) * (size_t)iters * N, hipMemcpyDeviceToHost));
  if (rotated) HIP_TRY(hipMemcpy(rotated, d_rot.p, sizeof(double) * 3 * (size_t)E, hipMemcpyDeviceToHost));
  if (axes_out) std::memcpy(axes_out, axes.data(), sizeof(double) * axes.size());
  stats.weights_ms = ms_since(t_weight);
  for (int it = 0; it < iters; ++it) { stats.source_steps += steps[2 * it]; stats.argmax_steps += steps[2 * it + 1]; }
  stats.lds_route = lds ? 1 : 0;
  stats.order_threads = threads;
  stats.total_ms = ms_since(t_start);
  g_stats = stats;
  return 0;
}

extern "C" int theia_hip_translation_filter_last_stats(theia_translation_filter_stats* out) {
  if (!out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out = g_stats;
  return 0;
}

extern "C" int theia_hip_filter_view_pairs_from_orientation(int32_t n_views, int32_t n_pairs, const int32_t* pairs,
                                                            const double* orientations, const uint8_t* has_orientation,
                                                            const double* rotation_2,
                                                            double max_relative_rotation_difference_degrees,
                                                            uint8_t* removed) {
  const int N = n_views, E = n_pairs;
  if (N < 0 || E < 0 || !removed || (E > 0 && (!pairs || !orientations || !rotation_2)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument or negative count");
  if (!(max_relative_rotation_difference_degrees >= 0.0))   // CHECK_GE(max_relative_rotation_difference_degrees, 0.0)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the angle is negative or NaN");
  int rc = check_pairs(N, E, pairs);
  if (rc) return rc;
  if (E == 0) return 0;
  const double rad = max_relative_rotation_difference_degrees * (M_PI / 180.0);   // DegToRad (util/util.h)
  if ((rc = thip::ensure_device())) return rc;
  DevBuf<int2> d_pairs;
  DevBuf<double> d_aa, d_rel;
  DevBuf<uint8_t> d_has, d_removed;
  if ((rc = d_pairs.up(pairs, E)) || (rc = d_aa.up(orientations, 3 * (size_t)N)) || (rc = d_rel.up(rotation_2, 3 * (size_t)E)) ||
      (has_orientation && (rc = d_has.up(has_orientation, N))) || (rc = d_removed.alloc(E)))
    return rc;
  k_orientation_filter<<<grid_of(E, kThreads), kThreads>>>(E, d_pairs.p, d_aa.p, has_orientation ? d_has.p : nullptr, d_rel.p, rad * rad,
                                                          d_removed.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(removed, d_removed.p, (size_t)E, hipMemcpyDeviceToHost));
  return 0;
}
