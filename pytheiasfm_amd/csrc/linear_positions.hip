// linear_positions.hip -- LinearPositionEstimator (global_pose_estimation/linear_position_estimator.cc:67-473,
// compute_triplet_baseline_ratios.cc:52-157, math/graph/triplet_extractor.h, triangulation.cc:130-157, 236-250; Jiang, Cui,
// Tan, "A Global Linear Method for Camera Pose Registration", ICCV 2013): global positions from the global orientations,
// the view pairs' relative poses and the tracks' normalised features, on the device in FP64.
//
// Every triangle (a < b < c) of the view graph gets two baseline ratios from the tracks its three views share: each such
// track is triangulated by the midpoint method in each of the pairs (a, b), (a, c), (b, c), and the medians of
// depth1_12 / depth1_13 and depth2_12 / depth2_23 give baseline = (1, m1, m2).  With the rotations between the three
// global translation directions (FromTwoVectors) a triangle gives three 3-row constraints on (c_a, c_b, c_c)
// (:396-422); the normal equations H = sum C' C on the 3 x 3 blocks of the views, without the held view, are a dense
// view-by-view matrix, and the positions are the eigenvector of its smallest eigenvalue.
//
// Stages:
//   host            the refusals; the CSR of every view's higher-numbered neighbours, sorted, with the edge index (from the
//                   incidence lists of view_graph_plan.h); the per-view lists of (track, observation), sorted by track
//   k_triplet_count one wavefront per edge (a, b) in sorted order: the lanes stride over N+(b) and look each c up in N+(a)
//                   by binary search
//   k_exclusive_scan one workgroup: the offsets of the edges' segments of the triangle list
//   k_triplet_fill  the same walk; every round of 64 is compacted by ballot and popcount prefix, so a segment ascends in c:
//                   every triangle once, the list lexicographic in (a, b, c), with its three edge indices
//   k_baseline_ratios  the hot kernel, one wavefront per triangle: the lanes stride over the shortest of the three views'
//                   lists and binary-search the other two; per common track three gated midpoint solves (a 3 x 3 LLT in
//                   registers per pair; the pairs' R_2 and position_2 once per wavefront, in LDS); the valid ratio pairs
//                   are compacted into the triangle's segment of a scratch array (sized from a prefix sum of
//                   min(len_a, len_b, len_c); triangles go in chunks of at most kScratchSlots slots), then the two
//                   elements of rank k / 2 by a radix select on the bit patterns of the positive doubles, eight passes
//                   of eight bits over an LDS histogram per wavefront (integer LDS atomics: the counts do not depend on
//                   their order)
//   host            the triangles without ratios leave; union-find over the edges of the others, the largest component;
//                   the counts, the view index, w = 1 / sqrt(min count); the blocks' item lists (smallest_eigenvector.h)
//   k_triplet_items one thread per used triangle: the three rotations, the nine constraint blocks, the six block sums
//                   sum_rows Ci' Cj (i <= j), rows in the reference's order
//   k_blocks, k_shift, dense_cholesky_factor, k_iterate, k_sign_vote   as in ligt_positions.hip
//
// Determinism: no floating-point atomics.  The ratios are compacted in track order, a selection is exact, every entry of
// H is a sum in triangle order by one owner.  Two runs on one input are bit-identical.
#include "smallest_eigenvector.h"
#include "view_graph_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <climits>
#include <numeric>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kShiftMultiple = 1.0;           // mu = kShiftMultiple * n * eps * max diag H, as in 3.6f
// ratio scratch: two doubles per slot, a slot per possible common track of a triangle of the chunk: 256 MiB at most
constexpr long long kScratchSlots = 1LL << 24;

// position of `key` in the ascending list[lo, hi), or -1
__device__ __forceinline__ int find_in(const int* __restrict__ list, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int v = list[mid];
    if (v == key) return mid;
    if (v < key) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// up_off [n + 1], up_nbr / up_row [E]: sorted edge s is (up_row[s], up_nbr[s]); N+(v) = up_nbr[up_off[v] .. up_off[v + 1])
__global__ __launch_bounds__(kThreads) void k_triplet_count(int E, const int* __restrict__ up_off, const int* __restrict__ up_row,
                                                            const int* __restrict__ up_nbr, int* __restrict__ count) {
  const int s = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= E) return;   // wave-uniform
  const int a = up_row[s], b = up_nbr[s];
  const int a0 = up_off[a], a1 = up_off[a + 1], b0 = up_off[b], b1 = up_off[b + 1];
  int found = 0;
  for (int j = b0 + lane; j < b1; j += 64) found += find_in(up_nbr, a0, a1, up_nbr[j]) >= 0 ? 1 : 0;
  const int total = wave_sum_butterfly(found);
  if (lane == 0) count[s] = total;
}

// off [n + 1] = exclusive prefix sums of count [n]; one workgroup, every thread a contiguous piece
__global__ __launch_bounds__(kThreads) void k_exclusive_scan(int n, const int* __restrict__ count, long long* __restrict__ off) {
  __shared__ long long part[kThreads];
  const int per = (n + kThreads - 1) / kThreads;
  const int i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int k = 0; k < kThreads; ++k) { const long long t = part[k]; part[k] = run; run += t; }
    off[n] = run;
  }
  __syncthreads();
  long long run = part[threadIdx.x];
  for (int i = i0; i < i1; ++i) { off[i] = run; run += count[i]; }
}

__global__ __launch_bounds__(kThreads) void k_triplet_fill(int E, const int* __restrict__ up_off, const int* __restrict__ up_row,
                                                           const int* __restrict__ up_nbr, const int* __restrict__ up_edge,
                                                           const long long* __restrict__ off, int* __restrict__ tri,
                                                           int* __restrict__ tri_edge) {
  const int s = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= E) return;   // wave-uniform
  const int a = up_row[s], b = up_nbr[s];
  const int a0 = up_off[a], a1 = up_off[a + 1], b0 = up_off[b], b1 = up_off[b + 1];
  long long base = off[s];
  const long long end = off[s + 1];
  for (int j0 = b0; j0 < b1; j0 += 64) {   // wave-uniform bounds
    const int j = j0 + lane;
    int pos = -1, c = 0;
    if (j < b1) { c = up_nbr[j]; pos = find_in(up_nbr, a0, a1, c); }
    const unsigned long long m = __ballot(pos >= 0);
    const long long k = base + __popcll(m & ((1ull << lane) - 1ull));
    if (pos >= 0 && k < end) {
      tri[3 * k] = a; tri[3 * k + 1] = b; tri[3 * k + 2] = c;
      tri_edge[3 * k] = up_edge[s]; tri_edge[3 * k + 1] = up_edge[pos]; tri_edge[3 * k + 2] = up_edge[j];
    }
    base += __popcll(m);
  }
}

// TriangulateMidpoint of the rays (0, d0) and (o1, d1), gated by SufficientTriangulationAngle: the depths |p| and
// |p - o1|.  False: d0 . d1 >= cos_min, or a pivot of the LLT of (I - d0 d0') + (I - d1 d1') is not positive.
__device__ __forceinline__ bool midpoint_depths(const double* d0, const double* d1, const double* o1, double cos_min,
                                                double* dep0, double* dep1) {
  const double c = (d0[0] * d1[0] + d0[1] * d1[1]) + d0[2] * d1[2];
  bool ok = c < cos_min;
  const double a00 = (1.0 - d0[0] * d0[0]) + (1.0 - d1[0] * d1[0]);
  const double a10 = (0.0 - d0[1] * d0[0]) + (0.0 - d1[1] * d1[0]);
  const double a11 = (1.0 - d0[1] * d0[1]) + (1.0 - d1[1] * d1[1]);
  const double a20 = (0.0 - d0[2] * d0[0]) + (0.0 - d1[2] * d1[0]);
  const double a21 = (0.0 - d0[2] * d0[1]) + (0.0 - d1[2] * d1[1]);
  const double a22 = (1.0 - d0[2] * d0[2]) + (1.0 - d1[2] * d1[2]);
  const double s = (d1[0] * o1[0] + d1[1] * o1[1]) + d1[2] * o1[2];
  const double b0 = o1[0] - d1[0] * s, b1 = o1[1] - d1[1] * s, b2 = o1[2] - d1[2] * s;
  ok = ok && a00 > 0.0;
  const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
  const double p1 = a11 - l10 * l10;
  ok = ok && p1 > 0.0;
  const double l11 = sqrt(p1), l21 = (a21 - l20 * l10) / l11;
  const double p2 = a22 - (l20 * l20 + l21 * l21);
  ok = ok && p2 > 0.0;
  const double l22 = sqrt(p2);
  const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = (b2 - (l20 * y0 + l21 * y1)) / l22;
  const double x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = (y0 - (l10 * x1 + l20 * x2)) / l00;
  *dep0 = sqrt((x0 * x0 + x1 * x1) + x2 * x2);
  const double e0 = x0 - o1[0], e1 = x1 - o1[1], e2 = x2 - o1[2];
  *dep1 = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
  return ok;
}

// the unit ray (x, y, 1) / |.| of observation o
__device__ __forceinline__ void unit_ray(const double* __restrict__ feat, int o, double* f) {
  const double x = feat[2 * (size_t)o], y = feat[2 * (size_t)o + 1];
  const double nrm = sqrt((x * x + y * y) + 1.0);
  f[0] = x / nrm; f[1] = y / nrm; f[2] = 1.0 / nrm;
}

// d = R' f (R row-major)
__device__ __forceinline__ void rot_t(const double* R, const double* f, double* d) {
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = (R[c] * f[0] + R[3 + c] * f[1]) + R[6 + c] * f[2];
}

// One wavefront per triangle t0 + w of the chunk.  vt_off [n + 1], vt_track / vt_obs: per view its (track, observation)
// pairs, ascending in track.  seg [count + 1]: the triangles' segments of r1 / r2.  Writes baselines [3] and valid [1]
// per triangle: (1, m1, m2) and k, or zeros.  Every wavefront runs the eight select passes, so that the workgroup's
// barriers are uniform; a wavefront without a triangle or without a ratio has nothing to count in them.
__global__ __launch_bounds__(kThreads) void k_baseline_ratios(int t0, int count, const int* __restrict__ tri,
                                                              const int* __restrict__ tri_edge, const int* __restrict__ vt_off,
                                                              const int* __restrict__ vt_track, const int* __restrict__ vt_obs,
                                                              const double* __restrict__ feat, const double* __restrict__ rel_rot,
                                                              const double* __restrict__ rel_pos, double cos_min,
                                                              const long long* __restrict__ seg, double* __restrict__ r1,
                                                              double* __restrict__ r2, double* __restrict__ baselines,
                                                              int* __restrict__ valid) {
  __shared__ double pair_R[kWaves][3][9];
  __shared__ double pair_o[kWaves][3][3];
  __shared__ unsigned hist[kWaves][2][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = blockIdx.x * kWaves + wv;
  const bool active = w < count;   // wave-uniform
  const int t = t0 + (active ? w : 0);
  int k = 0;                       // valid ratio pairs of this triangle
  long long s0 = 0;
  if (active) {
    if (lane < 3) {
      const int e = tri_edge[3 * (size_t)t + lane];
      double R[9];
      rsc::angle_axis_to_rot(rel_rot + 3 * (size_t)e, R);
#pragma unroll
      for (int q = 0; q < 9; ++q) pair_R[wv][lane][q] = R[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) pair_o[wv][lane][q] = rel_pos[3 * (size_t)e + q];
    }
  }
  __syncthreads();
  if (active) {
    s0 = seg[w];
    // the three views' lists: x is the shortest (the first of equal lengths), y and z the other two in view order
    const int va = tri[3 * (size_t)t], vb = tri[3 * (size_t)t + 1], vc = tri[3 * (size_t)t + 2];
    const int lo_a = vt_off[va], lo_b = vt_off[vb], lo_c = vt_off[vc];
    const int len_a = vt_off[va + 1] - lo_a, len_b = vt_off[vb + 1] - lo_b, len_c = vt_off[vc + 1] - lo_c;
    int x = 0, len_x = len_a;
    if (len_b < len_x) { x = 1; len_x = len_b; }
    if (len_c < len_x) { x = 2; len_x = len_c; }
    // selects, not indexed arrays: those would live in scratch memory
    const int lo_x = x == 0 ? lo_a : (x == 1 ? lo_b : lo_c);
    const int lo_y = x == 0 ? lo_b : lo_a, len_y = x == 0 ? len_b : len_a;
    const int lo_z = x == 2 ? lo_b : lo_c, len_z = x == 2 ? len_b : len_c;
    for (int j0 = 0; j0 < len_x; j0 += 64) {   // wave-uniform bounds
      const int j = j0 + lane;
      bool ok = false;
      double q1 = 0.0, q2 = 0.0;
      if (j < len_x) {
        const int track = vt_track[lo_x + j];
        const int py = find_in(vt_track, lo_y, lo_y + len_y, track);
        const int pz = py >= 0 ? find_in(vt_track, lo_z, lo_z + len_z, track) : -1;
        if (pz >= 0) {
          const int ox = vt_obs[lo_x + j], oy = vt_obs[py], oz = vt_obs[pz];
          double fa[3], fb[3], fc[3], d1[3];
          unit_ray(feat, x == 0 ? ox : oy, fa);
          unit_ray(feat, x == 1 ? ox : (x == 0 ? oy : oz), fb);
          unit_ray(feat, x == 2 ? ox : oz, fc);
          double d1_12, d2_12, d1_13, d3_13, d2_23, d3_23;
          rot_t(pair_R[wv][0], fb, d1);
          ok = midpoint_depths(fa, d1, pair_o[wv][0], cos_min, &d1_12, &d2_12);
          rot_t(pair_R[wv][1], fc, d1);
          ok = midpoint_depths(fa, d1, pair_o[wv][1], cos_min, &d1_13, &d3_13) && ok;
          rot_t(pair_R[wv][2], fc, d1);
          ok = midpoint_depths(fb, d1, pair_o[wv][2], cos_min, &d2_23, &d3_23) && ok;
          q1 = d1_12 / d1_13;
          q2 = d2_12 / d2_23;
          ok = ok && q1 > 0.0 && q1 < INFINITY && q2 > 0.0 && q2 < INFINITY;
        }
      }
      const unsigned long long m = __ballot(ok);
      if (ok) {
        const long long dst = s0 + k + __popcll(m & ((1ull << lane) - 1ull));
        if (dst < seg[w + 1]) { r1[dst] = q1; r2[dst] = q2; }
      }
      k += __popcll(m);
    }
  }
  // the lanes read back what other lanes of the wavefront wrote: the barrier below orders it (and it is uniform)
  __threadfence_block();
  unsigned long long prefix[2] = {0ull, 0ull};
  unsigned rank[2] = {(unsigned)(k / 2), (unsigned)(k / 2)};
  unsigned long long mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { hist[wv][0][4 * lane + q] = 0u; hist[wv][1][4 * lane + q] = 0u; }
    __syncthreads();
    for (int i = lane; i < k; i += 64) {
      const unsigned long long b1 = (unsigned long long)__double_as_longlong(r1[s0 + i]);
      const unsigned long long b2 = (unsigned long long)__double_as_longlong(r2[s0 + i]);
      if ((b1 & mask) == prefix[0]) atomicAdd(&hist[wv][0][(unsigned)(b1 >> shift) & 255u], 1u);
      if ((b2 & mask) == prefix[1]) atomicAdd(&hist[wv][1][(unsigned)(b2 >> shift) & 255u], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      // the bin that holds the element of rank[which] among the candidates: an inclusive scan over the lanes' four bins
      unsigned bins[4], sum = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) { bins[q] = hist[wv][which][4 * lane + q]; sum += bins[q]; }
      unsigned incl = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = (unsigned)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
      }
      const unsigned excl = incl - sum;
      const unsigned long long hit = __ballot(k > 0 && rank[which] >= excl && rank[which] < incl);
      unsigned digit = 0u, below = 0u;
      if (hit != 0ull) {
        const int src = __ffsll((long long)hit) - 1;
        unsigned my_digit = 0u, my_below = excl;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (rank[which] < my_below + bins[q]) break;
          my_below += bins[q];
          my_digit = q + 1;
        }
        digit = 4u * (unsigned)src + (unsigned)__shfl((int)my_digit, src, 64);
        below = (unsigned)__shfl((int)my_below, src, 64);
      }
      prefix[which] |= (unsigned long long)digit << shift;
      rank[which] -= below;
    }
    mask |= 255ull << shift;
    __syncthreads();
  }
  if (active && lane == 0) {
    double* out = baselines + 3 * (size_t)t;
    out[0] = k > 0 ? 1.0 : 0.0;
    out[1] = k > 0 ? __longlong_as_double((long long)prefix[0]) : 0.0;
    out[2] = k > 0 ? __longlong_as_double((long long)prefix[1]) : 0.0;
    valid[t] = k;
  }
}

// Eigen's Quaterniond::FromTwoVectors(a, b).toRotationMatrix(), row-major.  Where the vectors are antiparallel
// (c < -1 + 1e-12; Eigen takes an SVD there) the rotation by pi about u = normalize(v0 x e_k), k the first component of
// v0 of the smallest magnitude: 2 u u' - I.
__device__ __forceinline__ void from_two_vectors(const double* a, const double* b, double* R) {
  const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  const double v0[3] = {a[0] / na, a[1] / na, a[2] / na}, v1[3] = {b[0] / nb, b[1] / nb, b[2] / nb};
  const double c = (v1[0] * v0[0] + v1[1] * v0[1]) + v1[2] * v0[2];
  if (c < -1.0 + 1e-12) {
    const double m0 = fabs(v0[0]), m1 = fabs(v0[1]), m2 = fabs(v0[2]);
    double u[3];
    if (m0 <= m1 && m0 <= m2) { u[0] = 0.0; u[1] = v0[2]; u[2] = -v0[1]; }        // v0 x e_0
    else if (m1 <= m2) { u[0] = -v0[2]; u[1] = 0.0; u[2] = v0[0]; }               // v0 x e_1
    else { u[0] = v0[1]; u[1] = -v0[0]; u[2] = 0.0; }                             // v0 x e_2
    const double nu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    u[0] /= nu; u[1] /= nu; u[2] /= nu;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) R[3 * r + q] = 2.0 * (u[r] * u[q]) - (r == q ? 1.0 : 0.0);
    return;
  }
  double axis[3];
  cross3(v0, v1, axis);
  const double s = sqrt((1.0 + c) * 2.0);
  const double x = axis[0] / s, y = axis[1] / s, z = axis[2] / s, w = s * 0.5;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// t = -R' p (R row-major)
__device__ __forceinline__ void minus_rot_t(const double* R, const double* p, double* t) {
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = -((R[c] * p[0] + R[3 + c] * p[1]) + R[6 + c] * p[2]);
}

// The two general blocks of a constraint row: plus = ((sp P - Q' / sq) + I) w, minus = ((Q' / sq - sp P) + I) w.
__device__ __forceinline__ void row_blocks(const double* P, double sp, const double* Q, double sq, double w, double* plus,
                                           double* minus) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double id = r == c ? 1.0 : 0.0;
      const double p = sp * P[3 * r + c], q = Q[3 * c + r] / sq;
      plus[3 * r + c] = ((p - q) + id) * w;
      minus[3 * r + c] = ((q - p) + id) * w;
    }
}

// One thread per used triangle u (triangle used[u] of the list): items 6 u .. 6 u + 5 = sum over the three constraint
// rows of Ci' Cj for (i, j) = (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2).  The rows (:396-422), with I2 = -2 w I:
//   [ (-s201 r201 + r012' / s012 + I) w,  (s201 r201 - r012' / s012 + I) w,  I2 ]
//   [ (-r201' / s201 + s120 r120 + I) w,  I2,  (r201' / s201 - s120 r120 + I) w ]
//   [ I2,  (-s012 r012 + r120' / s120 + I) w,  (s012 r012 - r120' / s120 + I) w ]
__global__ __launch_bounds__(kThreads) void k_triplet_items(int num_used, const int* __restrict__ used,
                                                            const double* __restrict__ weight, const int* __restrict__ tri,
                                                            const int* __restrict__ tri_edge, const double* __restrict__ baselines,
                                                            const double* __restrict__ R, const double* __restrict__ rel_pos,
                                                            double* __restrict__ items) {
  const int u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= num_used) return;
  const int t = used[u];
  const double w = weight[u];
  const double* Ra = R + 9 * (size_t)tri[3 * (size_t)t];
  const double* Rb = R + 9 * (size_t)tri[3 * (size_t)t + 1];
  double t01[3], t02[3], t12[3], n01[3], n02[3], n12[3];
  minus_rot_t(Ra, rel_pos + 3 * (size_t)tri_edge[3 * (size_t)t], t01);
  minus_rot_t(Ra, rel_pos + 3 * (size_t)tri_edge[3 * (size_t)t + 1], t02);
  minus_rot_t(Rb, rel_pos + 3 * (size_t)tri_edge[3 * (size_t)t + 2], t12);
#pragma unroll
  for (int q = 0; q < 3; ++q) { n01[q] = -t01[q]; n02[q] = -t02[q]; n12[q] = -t12[q]; }
  double r012[9], r201[9], r120[9];
  from_two_vectors(t12, n01, r012);
  from_two_vectors(t01, t02, r201);
  from_two_vectors(n02, n12, r120);
  const double b0 = baselines[3 * (size_t)t], b1 = baselines[3 * (size_t)t + 1], b2 = baselines[3 * (size_t)t + 2];
  const double s012 = b0 / b2, s201 = b1 / b0, s120 = b2 / b1;
  // C[row][col]
  double C[3][3][9];
  const double i2 = -2.0 * w;
#pragma unroll
  for (int q = 0; q < 9; ++q) { const double d = (q % 4 == 0) ? i2 : 0.0; C[0][2][q] = d; C[1][1][q] = d; C[2][0][q] = d; }
  row_blocks(r201, s201, r012, s012, w, C[0][1], C[0][0]);
  row_blocks(r120, s120, r201, s201, w, C[1][0], C[1][2]);
  row_blocks(r012, s012, r120, s120, w, C[2][2], C[2][1]);
  double* out = items + 54 * (size_t)u;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      double T0[9], T1[9], T2[9], S[9];
      atb(C[0][i], C[0][j], T0);
      atb(C[1][i], C[1][j], T1);
      atb(C[2][i], C[2][j], T2);
#pragma unroll
      for (int q = 0; q < 9; ++q) S[q] = (T0[q] + T1[q]) + T2[q];
      store9(out, S);
      out += 9;
    }
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_linear_triplet_positions(
    int32_t num_views, const double* orientations, int32_t num_edges, const int32_t* edges, const double* relative_rotations,
    const double* relative_translations, int32_t num_tracks, const int32_t* track_offsets, const int32_t* obs_view,
    const double* obs_feature, const theia_linear_triplet_options* options, double* positions_out, uint8_t* estimated_out,
    int32_t triplet_capacity, int32_t* triplets_out, uint8_t* triplet_state_out, double* baselines_out, double* system_out,
    int32_t* system_index_out, theia_linear_triplet_summary* summary) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, T = num_tracks, E = num_edges;
  theia_linear_triplet_options o{1000, 0, 1e-8};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations || !positions_out || !estimated_out || !summary)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or a null output");
  if (E < 3 || !edges || !relative_rotations || !relative_translations)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "fewer than 3 view pairs, or view pairs without their arrays");
  if (T < 0 || !track_offsets || (T > 0 && (!obs_view || !obs_feature)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "tracks without their arrays");
  if (triplet_capacity < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "triplet_capacity must be >= 0");
  if (o.max_power_iterations <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_power_iterations must be > 0");
  if (!(o.eigensolver_threshold > 0.0) || !std::isfinite(o.eigensolver_threshold))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "eigensolver_threshold must be positive and finite");
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= n || j < 0 || j >= n)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view pair %d names view %d of %d", e, i < 0 || i >= n ? i : j, n);
    if (i >= j) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view pair %d is (%d, %d): first must be < second", e, i, j);
  }
  if (track_offsets[0] < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets must start at >= 0");
  for (int t = 0; t < T; ++t)
    if (track_offsets[t + 1] < track_offsets[t])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets decrease at track %d", t);
  const int num_obs = track_offsets[T];
  // the per-view (track, observation) lists: tracks in order, so every list ascends in track
  std::vector<int> vt_off(n + 1, 0), vt_track, vt_obs;
  {
    std::vector<int> seen(n, -1);
    for (int t = 0; t < T; ++t)
      for (int k = track_offsets[t]; k < track_offsets[t + 1]; ++k) {
        const int v = obs_view[k];
        if (v < 0 || v >= n) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %d names view %d of %d", k, v, n);
        if (seen[v] == t) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track %d names view %d twice", t, v);
        seen[v] = t;
        ++vt_off[v + 1];
      }
    for (int v = 0; v < n; ++v) vt_off[v + 1] += vt_off[v];
    vt_track.resize(std::max(1, vt_off[n]));
    vt_obs.resize(std::max(1, vt_off[n]));
    std::vector<int> fill(vt_off.begin(), vt_off.end() - 1);
    for (int t = 0; t < T; ++t)
      for (int k = track_offsets[t]; k < track_offsets[t + 1]; ++k) {
        const int at = fill[obs_view[k]]++;
        vt_track[at] = t;
        vt_obs[at] = k;
      }
  }
  // N+(v): the incident edges on which v is the first view (view_graph_plan.h lists them in edge order), sorted by the
  // second view; sorted edge s = position in this CSR
  std::vector<int> up_off(n + 1, 0), up_row(E), up_nbr(E), up_edge(E);
  {
    ViewGraphPlan plan;
    fill_view_graph_lists(n, std::vector<uint8_t>(n, 0), E, edges, &plan);
    std::vector<std::pair<int, int>> nb;   // (second view, edge)
    int s = 0;
    for (int v = 0; v < n; ++v) {
      nb.clear();
      for (int k = plan.inc_off[v]; k < plan.inc_off[v + 1]; ++k)
        if (!(plan.inc[k] & 1)) nb.emplace_back(edges[2 * (plan.inc[k] >> 1) + 1], plan.inc[k] >> 1);
      std::sort(nb.begin(), nb.end());
      for (size_t k = 0; k < nb.size(); ++k) {
        if (k && nb[k].first == nb[k - 1].first)
          return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view pair (%d, %d) is listed twice", v, nb[k].first);
        up_row[s] = v; up_nbr[s] = nb[k].first; up_edge[s] = nb[k].second;
        ++s;
      }
      up_off[v + 1] = s;
    }
  }

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  theia_linear_triplet_summary sm{};
  hipStream_t st = nullptr;
  DevBuf<double> d_aa, d_feat, d_R, d_rot, d_rel;
  DevBuf<int> d_up_off, d_up_row, d_up_nbr, d_up_edge, d_vt_off, d_vt_track, d_vt_obs, d_count;
  DevBuf<long long> d_off;
  DevBuf<int2> d_edges;
  if ((rc = d_aa.up(orientations, 3 * (size_t)n)) || (rc = d_feat.up(obs_feature, 2 * (size_t)num_obs)) ||
      (rc = d_R.alloc(9 * (size_t)n)) || (rc = d_rot.up(relative_rotations, 3 * (size_t)E)) ||
      (rc = d_rel.up(relative_translations, 3 * (size_t)E)) || (rc = d_edges.up(edges, E)) ||
      (rc = d_up_off.up(up_off.data(), n + 1)) || (rc = d_up_row.up(up_row.data(), E)) ||
      (rc = d_up_nbr.up(up_nbr.data(), E)) || (rc = d_up_edge.up(up_edge.data(), E)) ||
      (rc = d_vt_off.up(vt_off.data(), n + 1)) || (rc = d_vt_track.up(vt_track.data(), vt_track.size())) ||
      (rc = d_vt_obs.up(vt_obs.data(), vt_obs.size())) || (rc = d_count.alloc(E)) || (rc = d_off.alloc((size_t)E + 1)))
    return rc;
  k_rotations<kThreads><<<grid_of(n, kThreads), kThreads, 0, st>>>(n, d_aa.p, d_R.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  sm.setup_ms = ms_since(t_start);

  // ---- the triangles
  const auto t_triplets = std::chrono::steady_clock::now();
  k_triplet_count<<<grid_of(E, kWaves), kThreads, 0, st>>>(E, d_up_off.p, d_up_row.p, d_up_nbr.p, d_count.p);
  k_exclusive_scan<<<1, kThreads, 0, st>>>(E, d_count.p, d_off.p);
  HIP_TRY(hipGetLastError());
  long long total = 0;
  HIP_TRY(hipMemcpy(&total, d_off.p + E, sizeof(long long), hipMemcpyDeviceToHost));
  if (total == 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the view pairs form no triangle");
  if (total > INT32_MAX / 3) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%lld triangles: too many for the triangle list", total);
  const int Tn = (int)total;
  DevBuf<int> d_tri, d_tri_edge, d_valid;
  DevBuf<double> d_base;
  if ((rc = d_tri.alloc(3 * (size_t)Tn)) || (rc = d_tri_edge.alloc(3 * (size_t)Tn)) || (rc = d_valid.alloc(Tn)) ||
      (rc = d_base.alloc(3 * (size_t)Tn)))
    return rc;
  k_triplet_fill<<<grid_of(E, kWaves), kThreads, 0, st>>>(E, d_up_off.p, d_up_row.p, d_up_nbr.p, d_up_edge.p, d_off.p,
                                                         d_tri.p, d_tri_edge.p);
  HIP_TRY(hipGetLastError());
  std::vector<int> tri(3 * (size_t)Tn), tri_edge(3 * (size_t)Tn);
  HIP_TRY(hipMemcpy(tri.data(), d_tri.p, sizeof(int) * tri.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tri_edge.data(), d_tri_edge.p, sizeof(int) * tri_edge.size(), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < tri.size(); ++k)
    if (tri[k] < 0 || tri[k] >= n || tri_edge[k] < 0 || tri_edge[k] >= E)
      return set_error(THEIA_HIP_ERR_INTERNAL, "triangle %zu of the list is out of range", k / 3);
  sm.num_triplets = Tn;
  sm.triplets_ms = ms_since(t_triplets);

  // ---- the baseline ratios, in chunks of at most kScratchSlots possible common tracks
  const auto t_ratios = std::chrono::steady_clock::now();
  std::vector<int> valid(Tn);
  {
    auto slots = [&](int t) {
      int m = INT_MAX;
      for (int q = 0; q < 3; ++q) m = std::min(m, vt_off[tri[3 * (size_t)t + q] + 1] - vt_off[tri[3 * (size_t)t + q]]);
      return (long long)m;
    };
    long long most = 0, longest = 0;   // the largest chunk's slots and triangles
    for (int t0 = 0; t0 < Tn;) {
      long long run = 0;
      int t1 = t0;
      while (t1 < Tn && (t1 == t0 || run + slots(t1) <= kScratchSlots)) run += slots(t1++);
      if (run > kScratchSlots)
        return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "triangle %d alone has %lld possible common tracks: over the scratch budget", t0, run);
      most = std::max(most, run);
      longest = std::max<long long>(longest, t1 - t0);
      t0 = t1;
    }
    DevBuf<double> d_r1, d_r2;
    DevBuf<long long> d_seg;
    if ((rc = d_r1.alloc((size_t)most)) || (rc = d_r2.alloc((size_t)most)) || (rc = d_seg.alloc((size_t)longest + 1))) return rc;
    const double cos_min = std::cos(2.0 * M_PI / 180.0);   // kMinTriangulationAngle = 2 degrees
    std::vector<long long> seg;
    for (int t0 = 0; t0 < Tn;) {
      seg.assign(1, 0);
      int t1 = t0;
      while (t1 < Tn && (t1 == t0 || seg.back() + slots(t1) <= kScratchSlots)) { seg.push_back(seg.back() + slots(t1)); ++t1; }
      HIP_TRY(hipMemcpyAsync(d_seg.p, seg.data(), sizeof(long long) * seg.size(), hipMemcpyHostToDevice, st));
      k_baseline_ratios<<<grid_of(t1 - t0, kWaves), kThreads, 0, st>>>(t0, t1 - t0, d_tri.p, d_tri_edge.p, d_vt_off.p,
                                                                      d_vt_track.p, d_vt_obs.p, d_feat.p, d_rot.p, d_rel.p,
                                                                      cos_min, d_seg.p, d_r1.p, d_r2.p, d_base.p, d_valid.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(st));   // seg is reused by the next chunk
      t0 = t1;
    }
    HIP_TRY(hipMemcpy(valid.data(), d_valid.p, sizeof(int) * (size_t)Tn, hipMemcpyDeviceToHost));
  }
  sm.ratios_ms = ms_since(t_ratios);

  // ---- components over shared edges of the triangles that have ratios; the largest; counts, index, weights
  const auto t_assemble = std::chrono::steady_clock::now();
  std::vector<uint8_t> state(Tn, 0);
  std::vector<int> used;
  {
    std::vector<int> parent(E);
    std::iota(parent.begin(), parent.end(), 0);
    for (int t = 0; t < Tn; ++t) {
      if (valid[t] <= 0) { state[t] = 1; sm.triplets_without_ratios += 1; continue; }
      for (int q = 1; q < 3; ++q) {
        const int a = find_root(parent, tri_edge[3 * (size_t)t]), b = find_root(parent, tri_edge[3 * (size_t)t + q]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
      }
    }
    if (sm.triplets_without_ratios == Tn)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "none of the %d triangles has a track with valid baseline ratios", Tn);
    std::vector<int> size(E, 0);
    int best = -1;   // the first root to hold the largest count: its first triangle is the lexicographically first
    for (int t = 0; t < Tn; ++t)
      if (!state[t]) size[find_root(parent, tri_edge[3 * (size_t)t])] += 1;
    for (int t = 0; t < Tn; ++t) {
      if (state[t]) continue;
      const int r = find_root(parent, tri_edge[3 * (size_t)t]);
      if (best < 0 || size[r] > size[best]) best = r;
    }
    for (int t = 0; t < Tn; ++t) {
      if (state[t]) continue;
      if (find_root(parent, tri_edge[3 * (size_t)t]) == best) used.push_back(t);
      else { state[t] = 2; sm.triplets_in_other_components += 1; }
    }
  }
  const int U = sm.triplets_used = (int)used.size();
  std::vector<int> idx(n, -2), cnt(n, 0);
  int m = 0;
  for (int t : used)
    for (int q = 0; q < 3; ++q) {
      const int v = tri[3 * (size_t)t + q];
      cnt[v] += 1;
      if (idx[v] == -2) idx[v] = m++ - 1;
    }
  std::vector<double> weight(U);
  for (int u = 0; u < U; ++u) {
    const int* v = &tri[3 * (size_t)used[u]];
    weight[u] = 1.0 / std::sqrt((double)std::min({cnt[v[0]], cnt[v[1]], cnt[v[2]]}));
  }
  const int mf = m - 1;   // free views
  sm.num_views_in_system = m;
  if (6LL * U >= (1LL << 30)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%d used triangles: too many 3 x 3 items", U);

  SmallestEigenvector ev;
  if ((rc = ev.alloc(mf, system_out != nullptr))) return rc;

  BlockSegments seg;
  build_block_segments(mf, [&](auto&& emit) {
    for (int u = 0; u < U; ++u) {
      const int* v = &tri[3 * (size_t)used[u]];
      long long it = 6LL * u;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) emit(idx[v[i]], idx[v[j]], it++);
    }
  }, &seg);

  DevBuf<double> d_items, d_weight;
  DevBuf<int> d_idx, d_used;
  if ((rc = d_items.alloc(54 * (size_t)U)) || (rc = d_weight.up(weight.data(), U)) || (rc = d_used.up(used.data(), U)) ||
      (rc = d_idx.up(idx.data(), n)) || (rc = ev.upload(seg, st)))
    return rc;
  k_triplet_items<<<grid_of(U, kThreads), kThreads, 0, st>>>(U, d_used.p, d_weight.p, d_tri.p, d_tri_edge.p, d_base.p, d_R.p,
                                                            d_rel.p, d_items.p);
  if ((rc = ev.assemble(d_items.p, kShiftMultiple, st))) return rc;
  sm.assemble_ms = ms_since(t_assemble);

  if ((rc = ev.factor(st, &sm, summary))) return rc;

  // ---- inverse iteration, sign vote, scatter
  const auto t_eig = std::chrono::steady_clock::now();
  if ((rc = ev.iterate(o.max_power_iterations, o.eigensolver_threshold, st)) ||
      (rc = ev.vote(E, d_edges.p, d_idx.p, d_R.p, d_rel.p, st)) || (rc = ev.fetch()))
    return rc;
  std::vector<double> base;
  const int head = std::min(Tn, triplet_capacity);
  if (baselines_out && head > 0) {
    base.resize(3 * (size_t)head);
    HIP_TRY(hipMemcpy(base.data(), d_base.p, sizeof(double) * base.size(), hipMemcpyDeviceToHost));
  }
  sm.eig_ms = ms_since(t_eig);
  ev.scatter(n, idx, positions_out, estimated_out, system_out, system_index_out, &sm);
  if (triplets_out) std::copy(tri.begin(), tri.begin() + 3 * (size_t)head, triplets_out);
  if (triplet_state_out) std::copy(state.begin(), state.begin() + head, triplet_state_out);
  if (baselines_out) std::copy(base.begin(), base.end(), baselines_out);
  *summary = sm;
  return 0;
}
