// view_graph_pruning.hip -- the two view-graph prunings that need no global orientations:
//   FilterViewGraphCyclesByRotation (sfm/filter_view_graph_cycles_by_rotation.cc:54-145): every triangle a < b < c of the
//     view graph chains its three relative rotations, loop = R_bc * R_ab * R_ac' (:70-71), and its error is
//     RadToDeg(|RotationMatrixToAngleAxis(loop)|) (:72-79).  A pair stays when at least one of its triangles has an error
//     below the threshold (:132, strict); a pair in no triangle goes.  On the device.
//   RemoveDisconnectedViewPairs (sfm/view_graph/remove_disconnected_view_pairs.cc:48-95): only the largest connected
//     component stays.  On the host, a plain array union-find (view_graph_plan.h); it never touches a device.
//
// Kernels of the cycle filter
//   k_pair_matrices  one lane per pair: AngleAxisToRotationMatrix(rotation_2) in the pair's ASCENDING orientation, i.e.
//                    transposed when the pair is listed (b, a) with b > a; 9 doubles, row-major.
//   k_cycle_errors   one team of kTeam = 16 lanes per pair (lo, hi).  The host plan is the full adjacency as CSR, every list
//                    sorted by neighbour, entries (neighbour, pair index).  The lanes stride over the shorter of the two
//                    lists and bisect in the longer; a common neighbour c is one triangle.  The lane orders (lo, hi, c),
//                    which tells it which of the three pairs is (a, b), (a, c) and (b, c), reads the three matrices,
//                    forms the loop product and its angle, and keeps its running minimum and its count.  One team
//                    reduction (min, sum), then lane 0 stores the pair's minimum, count and verdict.
// Owner-writes: a triangle is visited from each of its three pairs, so no result is ever added to from two places and
// there is no atomic.  Minimum and integer sum do not depend on the order: two runs are byte-identical.
// A NaN error validates nothing (`err < m` is false), so the minimum ignores it; the triangle is still counted.
#include "rotation_maps.h"
#include "wave_reduce.h"
#include "device_util.h"
#include "view_graph_plan.h"

#include <cmath>
#include <limits>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
// lanes per pair in k_cycle_errors: 16 (a DPP row, four pairs per wavefront) or 64 (a wavefront).  16 is the faster at the
// two sizes timed (DESIGN.md 3.6o has both figures); -DTHEIA_CYCLE_TEAM=64 builds the other variant for
// scripts/gpu_time_view_graph_pruning.py.  Same outputs, byte for byte.
#ifndef THEIA_CYCLE_TEAM
#define THEIA_CYCLE_TEAM 16
#endif
constexpr int kTeam = THEIA_CYCLE_TEAM;
static_assert(kTeam == 64 || kTeam == 16, "a wavefront or a DPP row");
constexpr double kRadToDeg = 180.0 / M_PI;   // math/util.h:48

__global__ __launch_bounds__(kThreads) void k_pair_matrices(int E, const int2* __restrict__ pairs,
                                                            const double* __restrict__ rotation_2,
                                                            double* __restrict__ mats) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const double aa[3] = {rotation_2[3 * (size_t)e], rotation_2[3 * (size_t)e + 1], rotation_2[3 * (size_t)e + 2]};
  double R[9];
  rsc::angle_axis_to_rot(aa, R);
  const bool descending = pairs[e].x > pairs[e].y;
  double* out = mats + 9 * (size_t)e;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = descending ? R[3 * c + r] : R[3 * r + c];
}

// all-reduce over a team of TEAM lanes: the whole wave, or one DPP row of 16
template <int TEAM> __device__ __forceinline__ unsigned team_max_u32(unsigned v);
template <> __device__ __forceinline__ unsigned team_max_u32<64>(unsigned v) { return wave_max_u32(v); }
template <> __device__ __forceinline__ unsigned team_max_u32<16>(unsigned v) { return row16_max_u32(v); }
template <int TEAM> __device__ __forceinline__ int team_sum_i32(int v);
template <> __device__ __forceinline__ int team_sum_i32<64>(int v) { return wave_sum_butterfly(v); }
template <> __device__ __forceinline__ int team_sum_i32<16>(int v) { return row16_sum_i32(v); }

// min over the team of values that are >= 0 or +inf (never NaN): such doubles order like their bit patterns, and the
// minimum of a pattern is the complement of the maximum of its complement.
template <int TEAM>
__device__ __forceinline__ double team_min_nonneg(double v) {
  const unsigned hi = ~(unsigned)__double2hiint(v), lo = ~(unsigned)__double2loint(v);
  const unsigned hm = team_max_u32<TEAM>(hi);
  const unsigned lm = team_max_u32<TEAM>(hi == hm ? lo : 0u);
  return __hiloint2double((int)~hm, (int)~lm);
}

// |RotationMatrixToAngleAxis(R)|: rsc::rot_to_angle_axis (rotation_maps.h), operation for operation, with its
// largest-diagonal branch written out per index.  That function picks the index at run time, which puts the matrix and
// the quaternion into scratch (80 bytes per lane here); with the index a template argument everything stays in registers.
struct Quat { double w, x, y, z; };
template <int I>
__device__ __forceinline__ Quat quat_by_diagonal(const double* R) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double q[4];
  double t = sqrt(R[I * 3 + I] - R[J * 3 + J] - R[K * 3 + K] + 1.0);
  q[I + 1] = 0.5 * t;
  t = 0.5 / t;
  q[0] = (R[K * 3 + J] - R[J * 3 + K]) * t;
  q[J + 1] = (R[J * 3 + I] + R[I * 3 + J]) * t;
  q[K + 1] = (R[K * 3 + I] + R[I * 3 + K]) * t;
  return Quat{q[0], q[1], q[2], q[3]};
}
__device__ __forceinline__ double rotation_angle(const double* R) {
  const double trace = R[0] + R[4] + R[8];
  Quat q;
  if (trace >= 0.0) {
    double t = sqrt(trace + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (R[7] - R[5]) * t; q.y = (R[2] - R[6]) * t; q.z = (R[3] - R[1]) * t;
  } else if (R[8] > (R[4] > R[0] ? R[4] : R[0])) {
    q = quat_by_diagonal<2>(R);
  } else if (R[4] > R[0]) {
    q = quat_by_diagonal<1>(R);
  } else {
    q = quat_by_diagonal<0>(R);
  }
  const double s2 = q.x * q.x + q.y * q.y + q.z * q.z;
  double aa[3];
  if (s2 > 0.0) {
    const double st = sqrt(s2), ct = q.w;
    const double two_theta = 2.0 * ((ct < 0.0) ? atan2(-st, -ct) : atan2(st, ct));
    const double k = two_theta / st;
    aa[0] = q.x * k; aa[1] = q.y * k; aa[2] = q.z * k;
  } else {
    aa[0] = q.x * 2.0; aa[1] = q.y * 2.0; aa[2] = q.z * 2.0;
  }
  return sqrt((aa[0] * aa[0] + aa[1] * aa[1]) + aa[2] * aa[2]);   // Eigen's norm()
}

// ComputeLoopRotationError (:54-80) on ascending matrices: (R_bc * R_ab) * R_ac', Eigen's left-to-right product.
__device__ __forceinline__ double loop_error_degrees(const double* __restrict__ Rab, const double* __restrict__ Rac,
                                                     const double* __restrict__ Rbc) {
  double T[9], L[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T[3 * r + c] = (Rbc[3 * r] * Rab[c] + Rbc[3 * r + 1] * Rab[3 + c]) + Rbc[3 * r + 2] * Rab[6 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) L[3 * r + c] = (T[3 * r] * Rac[3 * c] + T[3 * r + 1] * Rac[3 * c + 1]) + T[3 * r + 2] * Rac[3 * c + 2];
  return rotation_angle(L) * kRadToDeg;
}

// adj_off [N + 1], adj [2 E] = (neighbour, pair), every list ascending in the neighbour; mats [E][9] ascending.
template <int TEAM>
__global__ __launch_bounds__(kThreads) void k_cycle_errors(int E, const int2* __restrict__ pairs,
                                                           const long long* __restrict__ adj_off,
                                                           const int2* __restrict__ adj, const double* __restrict__ mats,
                                                           double threshold, double* __restrict__ min_err,
                                                           int* __restrict__ tri_count, uint8_t* __restrict__ removed) {
  const int e = blockIdx.x * (kThreads / TEAM) + threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
  if (e >= E) return;   // a whole team leaves together
  const int2 p = pairs[e];
  const int lo = min(p.x, p.y), hi = max(p.x, p.y);
  const long long a0 = adj_off[lo], a1 = adj_off[lo + 1], b0 = adj_off[hi], b1 = adj_off[hi + 1];
  const bool lo_short = a1 - a0 <= b1 - b0;
  const long long s0 = lo_short ? a0 : b0, s1 = lo_short ? a1 : b1, l0 = lo_short ? b0 : a0, l1 = lo_short ? b1 : a1;
  double m = INFINITY;
  int count = 0;
  for (long long k = s0 + lane; k < s1; k += TEAM) {
    const int2 sc = adj[k];
    const int c = sc.x;
    if (c == lo || c == hi) continue;   // the pair itself
    long long x = l0, y = l1;
    while (x < y) {
      const long long mid = (x + y) >> 1;
      if (adj[mid].x < c) x = mid + 1; else y = mid;
    }
    if (x == l1) continue;
    const int2 lc = adj[x];
    if (lc.x != c) continue;
    const int e_lo = lo_short ? sc.y : lc.y, e_hi = lo_short ? lc.y : sc.y;   // the pairs (lo, c) and (hi, c)
    // the triangle in ascending order (a, b, c'): which pair is (a, b), (a, c'), (b, c')
    const int ab = c > hi ? e : e_lo;
    const int ac = c < lo ? e_hi : (c < hi ? e : e_lo);
    const int bc = c < lo ? e : e_hi;
    const double err = loop_error_degrees(mats + 9 * (size_t)ab, mats + 9 * (size_t)ac, mats + 9 * (size_t)bc);
    if (err < m) m = err;
    ++count;
  }
  m = team_min_nonneg<TEAM>(m);
  count = team_sum_i32<TEAM>(count);
  if (lane == 0) {
    min_err[e] = m;
    tri_count[e] = count;
    removed[e] = m < threshold ? 0 : 1;
  }
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_filter_view_graph_cycles_by_rotation(int32_t n_views, int32_t n_pairs, const int32_t* pairs,
                                                              const double* rotation_2, double max_loop_error_degrees,
                                                              uint8_t* removed, double* min_loop_error_degrees,
                                                              int32_t* triangles_per_pair, int64_t* num_triangles) {
  const int N = n_views, E = n_pairs;
  if (N < 0 || E < 0 || (E > 0 && (!pairs || !rotation_2 || !removed)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument or negative count");
  int rc = check_pairs(N, E, pairs);
  if (rc) return rc;
  if (E == 0) {
    if (num_triangles) *num_triangles = 0;
    return 0;
  }

  // the full adjacency, every list ascending in the neighbour: the lists in pair order first, then every view in
  // ascending order hands itself to its neighbours
  std::vector<long long> adj_off((size_t)N + 1, 0);
  std::vector<int2> by_pair(2 * (size_t)E), adj(2 * (size_t)E);
  for (int e = 0; e < E; ++e) { ++adj_off[pairs[2 * e] + 1]; ++adj_off[pairs[2 * e + 1] + 1]; }
  for (int v = 0; v < N; ++v) adj_off[v + 1] += adj_off[v];
  {
    std::vector<long long> fill(adj_off.begin(), adj_off.end() - 1);
    for (int e = 0; e < E; ++e) {
      const int i = pairs[2 * e], j = pairs[2 * e + 1];
      by_pair[fill[i]++] = make_int2(j, e);
      by_pair[fill[j]++] = make_int2(i, e);
    }
    fill.assign(adj_off.begin(), adj_off.end() - 1);
    for (int v = 0; v < N; ++v)
      for (long long k = adj_off[v]; k < adj_off[v + 1]; ++k) adj[fill[by_pair[k].x]++] = make_int2(v, by_pair[k].y);
  }

  if ((rc = thip::ensure_device())) return rc;
  DevBuf<int2> d_pairs, d_adj;
  DevBuf<long long> d_adj_off;
  DevBuf<double> d_rel, d_mats, d_min;
  DevBuf<int> d_count;
  DevBuf<uint8_t> d_removed;
  if ((rc = d_pairs.up(pairs, E)) || (rc = d_rel.up(rotation_2, 3 * (size_t)E)) || (rc = d_adj_off.up(adj_off.data(), adj_off.size())) ||
      (rc = d_adj.up(adj.data(), adj.size())) || (rc = d_mats.alloc(9 * (size_t)E)) || (rc = d_min.alloc(E)) ||
      (rc = d_count.alloc(E)) || (rc = d_removed.alloc(E)))
    return rc;
  k_pair_matrices<<<grid_of(E, kThreads), kThreads>>>(E, d_pairs.p, d_rel.p, d_mats.p);
  k_cycle_errors<kTeam><<<grid_of(E, kThreads / kTeam), kThreads>>>(E, d_pairs.p, d_adj_off.p, d_adj.p, d_mats.p, max_loop_error_degrees,
                                                                   d_min.p, d_count.p, d_removed.p);
  HIP_TRY(hipGetLastError());
  std::vector<int> count((size_t)E);
  HIP_TRY(hipMemcpy(count.data(), d_count.p, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(removed, d_removed.p, (size_t)E, hipMemcpyDeviceToHost));
  if (min_loop_error_degrees) HIP_TRY(hipMemcpy(min_loop_error_degrees, d_min.p, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost));
  if (triangles_per_pair) std::copy(count.begin(), count.end(), triangles_per_pair);
  if (num_triangles) {
    int64_t visits = 0;
    for (int e = 0; e < E; ++e) visits += count[e];
    *num_triangles = visits / 3;   // every triangle was visited from each of its three pairs
  }
  return 0;
}

extern "C" int theia_hip_remove_disconnected_view_pairs(int32_t n_views, int32_t n_pairs, const int32_t* pairs,
                                                        uint8_t* removed_pairs, uint8_t* removed_views, int32_t* component) {
  const int N = n_views, E = n_pairs;
  if (N < 0 || E < 0 || (E > 0 && (!pairs || !removed_pairs || !removed_views)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument or negative count");
  int rc = check_pairs(N, E, pairs);
  if (rc) return rc;
  std::vector<int> root;   // the smallest view of every view's component
  if ((rc = view_graph_components(N, E, pairs, &root))) return rc;
  std::vector<uint8_t> named((size_t)N, 0);
  for (int e = 0; e < E; ++e) named[pairs[2 * e]] = named[pairs[2 * e + 1]] = 1;
  // the largest component by views (:62-69); among equals the one with the smallest view, which the ascending scan
  // with a strict comparison finds first
  std::vector<int> size((size_t)N, 0);
  for (int v = 0; v < N; ++v) if (named[v]) ++size[root[v]];
  int kept = -1, kept_size = 0;
  for (int v = 0; v < N; ++v) if (size[v] > kept_size) { kept = v; kept_size = size[v]; }
  for (int v = 0; v < N; ++v) {
    if (removed_views) removed_views[v] = named[v] && root[v] != kept ? 1 : 0;
    if (component) component[v] = named[v] ? root[v] : -1;
  }
  for (int e = 0; e < E; ++e) removed_pairs[e] = root[pairs[2 * e]] != kept ? 1 : 0;
  return 0;
}
