// covisibility.hip -- from a reconstruction back to a view graph and on to dense stereo:
//   ViewGraphFromReconstruction (sfm/view_graph/view_graph_from_reconstruction.cc:41-105): an edge for every pair of
//     estimated views that share more than min_shared_tracks estimated tracks, with rotation_2 = log(R_j R_i'),
//     position_2 = R_i (c_j - c_i).normalized() and the count.
//   ViewSelectionMVSNet (mvs/view_selection_mvsnet.cc:39-125): for every view its best source views, ranked by the sum
//     over the common tracks of a Gaussian of the triangulation angle.
//   FindCommonTracksInViews (sfm/find_common_tracks_in_views.cc:58-88): the tracks all views of a query observe.
// The rules, the deviations and the refusals are stated in include/theia_hip.h; DESIGN.md 3.6w has the measurements.
//
// The host plan (Plan::build): the observations as two CSR forms, by view with every view's tracks ascending and by track
// with every track's views ascending, made by three counting passes (rows by view; those by track; those by view again).
//
// Kernels
//   k_covis_rows<EMIT>  one workgroup per row i.  Int32 counters for a window of columns j > i live in LDS; the lanes
//                       stride over view i's estimated tracks and walk each track's views inside the window, adding 1 with
//                       an LDS integer atomic.  Then every wave scans its quarter of the window 64 columns at a time
//                       (ballot + popcount), the four wave totals meet in LDS, and with EMIT the pairs are written in
//                       ascending j.  A row with more columns than one window takes further passes.  Run twice: the count
//                       pass gives the row sizes, the host scans them, the emit pass writes at the row's offset --
//                       owner-writes, no global atomic, the output order fixed.  Only j > i is counted: a variant
//                       that counted every column, rows of equal work at twice the work, was slower.
//   k_edge_data         one lane per edge: rotation_2 and position_2 through rotation_maps.h.
//   k_pair_scores       one team of 16 lanes (a DPP row) per pair, as k_cycle_errors (view_graph_pruning.hip): the lanes
//                       stride over the shorter sorted track list and bisect in the longer; a lane adds its terms in
//                       ascending order, then one fixed reduction over the row.
//   k_common_tracks<WRITE>  one team per query: the candidates are the shortest list, 16 at a time, each bisected in the
//                       other lists; the team's ballot places the hits in ascending order.  Count, host scan, write.
// No floating-point atomic anywhere in this file.
#include "rotation_maps.h"
#include "wave_reduce.h"
#include "device_util.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTeam = 16;
constexpr int kMaxWindow = THEIA_COVISIBILITY_DEFAULT_WINDOW;   // int32 counters: 32 KiB of LDS
constexpr double kRadToDeg = 180.0 / M_PI;

// the two CSR forms, device pointers
struct Csr {
  const long long* view_off;    // [V + 1]
  const int* view_track;        // [N] every view's tracks, ascending
  const long long* track_off;   // [T + 1]
  const int* track_view;        // [N] every track's views, ascending
};

// first position in [x, y) of the ascending list whose entry is not below key
__device__ __forceinline__ long long lower_bound(const int* __restrict__ list, long long x, long long y, long long key) {
  while (x < y) {
    const long long mid = (x + y) >> 1;
    if (list[mid] < key) x = mid + 1; else y = mid;
  }
  return x;
}

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_covis_rows(int V, int window, int min_shared, Csr g,
                                                         const uint8_t* __restrict__ view_est,
                                                         const uint8_t* __restrict__ track_est, int* __restrict__ row_count,
                                                         const long long* __restrict__ row_off, int2* __restrict__ pairs,
                                                         int* __restrict__ num_shared) {
  extern __shared__ int s_cnt[];   // [window]
  __shared__ int s_wave[kWaves];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (!view_est[i]) {   // the whole workgroup leaves
    if (!EMIT && tid == 0) row_count[i] = 0;
    return;
  }
  const long long t0 = g.view_off[i], t1 = g.view_off[i + 1];
  const long long out = EMIT ? row_off[i] : 0;
  int total = 0;
  for (long long w0 = (long long)i + 1; w0 < V; w0 += window) {
    const int wn = (int)min((long long)window, (long long)V - w0);
    for (int c = tid; c < wn; c += kThreads) s_cnt[c] = 0;
    __syncthreads();
    for (long long k = t0 + tid; k < t1; k += kThreads) {
      const int t = g.view_track[k];
      if (!track_est[t]) continue;
      const long long b1 = g.track_off[t + 1];
      for (long long x = lower_bound(g.track_view, g.track_off[t], b1, w0); x < b1; ++x) {
        const long long j = g.track_view[x];
        if (j >= w0 + wn) break;
        if (view_est[j]) atomicAdd(&s_cnt[j - w0], 1);
      }
    }
    __syncthreads();
    // every wave scans its contiguous share of the window, 64 columns at a time
    const int seg = ((wn + kThreads - 1) / kThreads) * 64;
    const int s0 = min(wv * seg, wn), s1 = min(s0 + seg, wn);
    int mine = 0;
    for (int b = s0; b < s1; b += 64) {
      const int c = b + lane;
      mine += __popcll(__builtin_amdgcn_ballot_w64(c < s1 && s_cnt[c] > min_shared));
    }
    if (lane == 0) s_wave[wv] = mine;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int v = s_wave[w];
      before += w < wv ? v : 0;
      all += v;
    }
    if (EMIT) {
      long long pos = out + total + before;
      for (int b = s0; b < s1; b += 64) {
        const int c = b + lane;
        const int n = c < s1 ? s_cnt[c] : 0;
        const bool hit = c < s1 && n > min_shared;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (hit) {
          const long long p = pos + __popcll(mask & ((1ull << lane) - 1ull));
          pairs[p] = make_int2(i, (int)(w0 + c));
          num_shared[p] = n;
        }
        pos += __popcll(mask);
      }
    }
    total += all;
    __syncthreads();   // the counters and s_wave are reused by the next window
  }
  if (!EMIT && tid == 0) row_count[i] = total;
}

// CreateTwoViewInfo (:41-60); cam_ext [V][6] = position | angle-axis
__global__ __launch_bounds__(kThreads) void k_edge_data(long long E, const int2* __restrict__ pairs,
                                                        const double* __restrict__ cam_ext, double* __restrict__ rotation_2,
                                                        double* __restrict__ position_2) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const double* ci = cam_ext + 6 * (size_t)pairs[e].x;
  const double* cj = cam_ext + 6 * (size_t)pairs[e].y;
  const double ai[3] = {ci[3], ci[4], ci[5]}, aj[3] = {cj[3], cj[4], cj[5]};
  double Ri[9], Rj[9];
  rsc::angle_axis_to_rot(ai, Ri);
  rsc::angle_axis_to_rot(aj, Rj);
  if (rotation_2) {
    double R[9], aa[3];   // R_j * R_i'
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (Rj[3 * r] * Ri[3 * c] + Rj[3 * r + 1] * Ri[3 * c + 1]) + Rj[3 * r + 2] * Ri[3 * c + 2];
    rsc::rot_to_angle_axis(R, aa);
    rotation_2[3 * e] = aa[0]; rotation_2[3 * e + 1] = aa[1]; rotation_2[3 * e + 2] = aa[2];
  }
  if (position_2) {
    const double d[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
    const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);   // no guard: coincident centres give NaN
    const double u[3] = {d[0] / n, d[1] / n, d[2] / n};
#pragma unroll
    for (int r = 0; r < 3; ++r) position_2[3 * e + r] = (Ri[3 * r] * u[0] + Ri[3 * r + 1] * u[1]) + Ri[3 * r + 2] * u[2];
  }
}

// sum over a DPP row of 16 lanes, the four row-local levels of wave_sum_butterfly(double): every lane gets the sum
__device__ __forceinline__ double row16_sum_f64(double v) {
  v += wr_dpp_d<0x128>(v);   // row_ror:8
  v += wr_dpp_d<0x124>(v);   // row_ror:4
  v += wr_dpp_d<0x4E>(v);    // quad_perm [2,3,0,1]
  v += wr_dpp_d<0xB1>(v);    // quad_perm [1,0,3,2]
  return v;
}

// ComputeAngleBetweenRays and ScoreFun (view_selection_mvsnet.cc:39-52) for the centres ci, cj and the point X [4]
__device__ __forceinline__ double mvsnet_term(const double* ci, const double* cj, const double* __restrict__ X, double theta0,
                                              double sigma1, double sigma2) {
  const double p[3] = {X[0] / X[3], X[1] / X[3], X[2] / X[3]};
  const double a[3] = {ci[0] - p[0], ci[1] - p[1], ci[2] - p[2]}, b[3] = {cj[0] - p[0], cj[1] - p[1], cj[2] - p[2]};
  const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  const double cos_angle = ((a[0] / na) * (b[0] / nb) + (a[1] / na) * (b[1] / nb)) + (a[2] / na) * (b[2] / nb);
  const double theta = kRadToDeg * acos(cos_angle);
  const double sigma = theta <= theta0 ? sigma1 : sigma2;
  const double d = theta - theta0;
  return exp(-(d * d) / (2.0 * (sigma * sigma)));
}

__global__ __launch_bounds__(kThreads) void k_pair_scores(long long E, const int2* __restrict__ pairs, Csr g,
                                                          const double* __restrict__ cam_ext, const double* __restrict__ points,
                                                          const uint8_t* __restrict__ track_mask, double theta0, double sigma1,
                                                          double sigma2, double* __restrict__ score, int* __restrict__ num_common) {
  const long long e = (long long)blockIdx.x * (kThreads / kTeam) + threadIdx.x / kTeam;
  const int lane = threadIdx.x % kTeam;
  if (e >= E) return;   // a whole team leaves together
  const int2 p = pairs[e];
  const int lo = min(p.x, p.y), hi = max(p.x, p.y);
  const long long a0 = g.view_off[lo], a1 = g.view_off[lo + 1], b0 = g.view_off[hi], b1 = g.view_off[hi + 1];
  const bool lo_short = a1 - a0 <= b1 - b0;
  const long long s0 = lo_short ? a0 : b0, s1 = lo_short ? a1 : b1, l0 = lo_short ? b0 : a0, l1 = lo_short ? b1 : a1;
  const double ci[3] = {cam_ext[6 * (size_t)lo], cam_ext[6 * (size_t)lo + 1], cam_ext[6 * (size_t)lo + 2]};
  const double cj[3] = {cam_ext[6 * (size_t)hi], cam_ext[6 * (size_t)hi + 1], cam_ext[6 * (size_t)hi + 2]};
  double sum = 0.0;
  int count = 0;
  for (long long k = s0 + lane; k < s1; k += kTeam) {
    const int t = g.view_track[k];
    if (track_mask && !track_mask[t]) continue;
    const long long x = lower_bound(g.view_track, l0, l1, t);
    if (x == l1 || g.view_track[x] != t) continue;
    sum += mvsnet_term(ci, cj, points + 4 * (size_t)t, theta0, sigma1, sigma2);
    ++count;
  }
  sum = row16_sum_f64(sum);
  count = row16_sum_i32(count);
  if (lane == 0) {
    score[e] = sum;
    num_common[e] = count;
  }
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_common_tracks(int Q, const long long* __restrict__ q_off,
                                                            const int* __restrict__ q_views, Csr g, int* __restrict__ count,
                                                            const long long* __restrict__ out_off, int* __restrict__ tracks) {
  const int q = blockIdx.x * (kThreads / kTeam) + threadIdx.x / kTeam, lane = threadIdx.x % kTeam;
  if (q >= Q) return;   // a whole team leaves together
  const long long a0 = q_off[q], a1 = q_off[q + 1];
  int best = q_views[a0];
  long long len = g.view_off[best + 1] - g.view_off[best];
  for (long long k = a0 + 1; k < a1; ++k) {   // the shortest list, the first of equals
    const int v = q_views[k];
    const long long l = g.view_off[v + 1] - g.view_off[v];
    if (l < len) { best = v; len = l; }
  }
  const long long s0 = g.view_off[best];
  const unsigned shift = (threadIdx.x & 63u) & ~(unsigned)(kTeam - 1);   // the team's first lane in its wave
  long long pos = WRITE ? out_off[q] : 0;
  int n = 0;
  for (long long b = 0; b < len; b += kTeam) {
    bool hit = b + lane < len;
    int t = 0;
    if (hit) {
      t = g.view_track[s0 + b + lane];
      for (long long k = a0; k < a1 && hit; ++k) {
        const int v = q_views[k];
        if (v == best) continue;
        const long long l1 = g.view_off[v + 1], x = lower_bound(g.view_track, g.view_off[v], l1, t);
        hit = x < l1 && g.view_track[x] == t;
      }
    }
    const unsigned mask = (unsigned)(__builtin_amdgcn_ballot_w64(hit) >> shift) & 0xFFFFu;
    if (WRITE && hit) tracks[pos + __popc(mask & ((1u << lane) - 1u))] = t;
    pos += __popc(mask);
    n += __popc(mask);
  }
  if (!WRITE && lane == 0) count[q] = n;
}

// ---------------------------------------------------------------------------------------------------------- host side

struct Observations {
  int V, T;
  long long N;
  const int32_t* view;
  const int32_t* track;
};

int check_observations(const Observations& o) {
  if (o.V < 0 || o.T < 0 || o.N < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if (o.N > 0 && (!o.view || !o.track)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null observation arrays");
  for (long long k = 0; k < o.N; ++k) {
    if (o.view[k] < 0 || o.view[k] >= o.V)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld names a view out of range", k);
    if (o.track[k] < 0 || o.track[k] >= o.T)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld names a track out of range", k);
  }
  return 0;
}

int check_score_parameters(double theta0, double sigma1, double sigma2) {
  if (std::isnan(theta0) || std::isnan(sigma1) || std::isnan(sigma2))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "theta0, sigma1 or sigma2 is NaN");
  if (sigma1 == 0.0 || sigma2 == 0.0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a sigma of 0");
  return 0;
}

// The two CSR forms on the host, then on the device.
struct Plan {
  std::vector<long long> view_off, track_off;
  std::vector<int> view_track, track_view;
  DevBuf<long long> d_view_off, d_track_off;
  DevBuf<int> d_view_track, d_track_view;
  DevBuf<uint8_t> d_view_est, d_track_est;
  DevBuf<double> d_cam, d_points;

  void build(const Observations& o) {
    const size_t N = (size_t)o.N;
    view_off.assign((size_t)o.V + 1, 0);
    track_off.assign((size_t)o.T + 1, 0);
    for (size_t k = 0; k < N; ++k) { ++view_off[o.view[k] + 1]; ++track_off[o.track[k] + 1]; }
    for (int v = 0; v < o.V; ++v) view_off[v + 1] += view_off[v];
    for (int t = 0; t < o.T; ++t) track_off[t + 1] += track_off[t];
    view_track.resize(N);
    track_view.resize(N);
    // rows by view (any order inside a view) -> by track, views ascending -> by view, tracks ascending.  Views are the
    // fewer: two of the three passes write through V cursors, only the middle one scatters over the T track cursors.
    std::vector<int> by_view(N);
    std::vector<long long> fill(view_off.begin(), view_off.end() - 1);
    for (size_t k = 0; k < N; ++k) by_view[fill[o.view[k]]++] = o.track[k];
    fill.assign(track_off.begin(), track_off.end() - 1);
    for (int v = 0; v < o.V; ++v)
      for (long long k = view_off[v]; k < view_off[v + 1]; ++k) track_view[fill[by_view[k]]++] = v;
    fill.assign(view_off.begin(), view_off.end() - 1);
    for (int t = 0; t < o.T; ++t)
      for (long long k = track_off[t]; k < track_off[t + 1]; ++k) view_track[fill[track_view[k]]++] = t;
  }

  int upload() {
    int rc;
    if ((rc = d_view_off.up(view_off.data(), view_off.size())) || (rc = d_track_off.up(track_off.data(), track_off.size())) ||
        (rc = d_view_track.up(view_track.data(), view_track.size())) || (rc = d_track_view.up(track_view.data(), track_view.size())))
      return rc;
    return 0;
  }
  // the flags, all ones for a NULL array
  static int upload_flags(DevBuf<uint8_t>* d, const uint8_t* flags, int n) {
    std::vector<uint8_t> f((size_t)n, 1);
    for (int k = 0; k < n && flags; ++k) f[k] = flags[k] ? 1 : 0;
    return d->up(f.data(), f.size());
  }
  Csr csr() const { return Csr{d_view_off.p, d_view_track.p, d_track_off.p, d_track_view.p}; }
};

int window_of(int column_window) { return column_window == 0 ? kMaxWindow : std::min(column_window, kMaxWindow); }

// The rows of the graph: the count pass, the scan, and when the count fits `capacity` (or capacity < 0: always) the emit
// pass into d_pairs / d_shared.  The plan and its flags are on the device.
int run_graph(const Plan& plan, int V, int min_shared, int window, long long capacity, DevBuf<int2>* d_pairs,
              DevBuf<int>* d_shared, long long* num_pairs) {
  int rc;
  DevBuf<int> d_row_count;
  DevBuf<long long> d_row_off;
  if ((rc = d_row_count.alloc((size_t)V)) || (rc = d_row_off.alloc((size_t)V))) return rc;
  const size_t lds = sizeof(int) * (size_t)window;
  k_covis_rows<false><<<V, kThreads, lds>>>(V, window, min_shared, plan.csr(), plan.d_view_est.p, plan.d_track_est.p,
                                            d_row_count.p, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  std::vector<int> row_count((size_t)V);
  HIP_TRY(hipMemcpy(row_count.data(), d_row_count.p, sizeof(int) * (size_t)V, hipMemcpyDeviceToHost));
  std::vector<long long> row_off((size_t)V);
  long long E = 0;
  for (int v = 0; v < V; ++v) { row_off[v] = E; E += row_count[v]; }
  *num_pairs = E;
  if (E == 0 || (capacity >= 0 && E > capacity)) return 0;
  if ((rc = d_pairs->alloc((size_t)E)) || (rc = d_shared->alloc((size_t)E))) return rc;
  HIP_TRY(hipMemcpy(d_row_off.p, row_off.data(), sizeof(long long) * (size_t)V, hipMemcpyHostToDevice));
  k_covis_rows<true><<<V, kThreads, lds>>>(V, window, min_shared, plan.csr(), plan.d_view_est.p, plan.d_track_est.p, nullptr,
                                           d_row_off.p, d_pairs->p, d_shared->p);
  HIP_TRY(hipGetLastError());
  return 0;
}

int run_scores(const Plan& plan, long long E, const int2* d_pairs, const uint8_t* d_mask, double theta0, double sigma1,
               double sigma2, double* d_score, int* d_common) {
  k_pair_scores<<<grid_of((size_t)E, kThreads / kTeam), kThreads>>>(E, d_pairs, plan.csr(), plan.d_cam.p, plan.d_points.p, d_mask,
                                                                    theta0, sigma1, sigma2, d_score, d_common);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_covisibility_graph(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                            const int32_t* obs_track, const uint8_t* view_estimated,
                                            const uint8_t* track_estimated, const double* cam_ext, int32_t min_shared_tracks,
                                            int32_t column_window, int64_t pair_capacity, int32_t* pairs, int32_t* num_shared,
                                            double* rotation_2, double* position_2, int64_t* num_pairs) {
  const Observations o{num_views, num_tracks, num_obs, obs_view, obs_track};
  int rc = check_observations(o);
  if (rc) return rc;
  if (min_shared_tracks < 0 || column_window < 0 || pair_capacity < 0)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative min_shared_tracks, column_window or pair_capacity");
  if (!num_pairs || (pair_capacity > 0 && (!pairs || !num_shared)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null output");
  const bool edge_data = rotation_2 || position_2;
  if (edge_data && num_views > 0 && !cam_ext)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "rotation_2 or position_2 asked for without cam_ext");
  if (num_views == 0 || num_obs == 0) {
    *num_pairs = 0;
    return 0;
  }
  Plan plan;
  plan.build(o);
  if ((rc = ensure_device())) return rc;
  if ((rc = plan.upload()) || (rc = Plan::upload_flags(&plan.d_view_est, view_estimated, num_views)) ||
      (rc = Plan::upload_flags(&plan.d_track_est, track_estimated, num_tracks)))
    return rc;
  DevBuf<int2> d_pairs;
  DevBuf<int> d_shared;
  long long E = 0;
  if ((rc = run_graph(plan, num_views, min_shared_tracks, window_of(column_window), pair_capacity, &d_pairs, &d_shared, &E)))
    return rc;
  if (E > 0 && E <= pair_capacity) {
    // everything that can fail runs before the first byte goes to the caller
    DevBuf<double> d_rot, d_pos;
    if (edge_data) {
      if ((rc = plan.d_cam.up(cam_ext, 6 * (size_t)num_views)) || (rotation_2 && (rc = d_rot.alloc(3 * (size_t)E))) ||
          (position_2 && (rc = d_pos.alloc(3 * (size_t)E))))
        return rc;
      k_edge_data<<<grid_of((size_t)E, kThreads), kThreads>>>(E, d_pairs.p, plan.d_cam.p, d_rot.p, d_pos.p);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(pairs, d_pairs.p, sizeof(int2) * (size_t)E, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(num_shared, d_shared.p, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost));
    if (rotation_2) HIP_TRY(hipMemcpy(rotation_2, d_rot.p, sizeof(double) * 3 * (size_t)E, hipMemcpyDeviceToHost));
    if (position_2) HIP_TRY(hipMemcpy(position_2, d_pos.p, sizeof(double) * 3 * (size_t)E, hipMemcpyDeviceToHost));
  }
  *num_pairs = E;
  return 0;
}

extern "C" int theia_hip_mvsnet_pair_scores(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                            const int32_t* obs_track, const double* cam_ext, const double* points,
                                            const uint8_t* track_mask, int64_t num_pairs, const int32_t* pairs, double theta0,
                                            double sigma1, double sigma2, double* score, int32_t* num_common) {
  const Observations o{num_views, num_tracks, num_obs, obs_view, obs_track};
  int rc = check_observations(o);
  if (rc) return rc;
  if (num_pairs < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if ((rc = check_score_parameters(theta0, sigma1, sigma2))) return rc;
  if (num_pairs > 0 && (!pairs || !score || !num_common || !cam_ext || (num_tracks > 0 && !points)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  for (int64_t e = 0; e < num_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    if (i < 0 || i >= num_views || j < 0 || j >= num_views)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %lld names a view out of range", (long long)e);
    if (i == j) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %lld names view %d twice", (long long)e, i);
  }
  if (num_pairs == 0) return 0;
  if (num_obs == 0) {
    std::fill(score, score + num_pairs, 0.0);
    std::fill(num_common, num_common + num_pairs, 0);
    return 0;
  }
  Plan plan;
  plan.build(o);
  if ((rc = ensure_device())) return rc;
  DevBuf<int2> d_pairs;
  DevBuf<uint8_t> d_mask;
  DevBuf<double> d_score;
  DevBuf<int> d_common;
  if ((rc = plan.upload()) || (rc = plan.d_cam.up(cam_ext, 6 * (size_t)num_views)) ||
      (rc = plan.d_points.up(points, 4 * (size_t)num_tracks)) || (rc = d_pairs.up(pairs, (size_t)num_pairs)) ||
      (track_mask && (rc = d_mask.up(track_mask, (size_t)num_tracks))) || (rc = d_score.alloc((size_t)num_pairs)) ||
      (rc = d_common.alloc((size_t)num_pairs)))
    return rc;
  if ((rc = run_scores(plan, num_pairs, d_pairs.p, track_mask ? d_mask.p : nullptr, theta0, sigma1, sigma2, d_score.p, d_common.p)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(score, d_score.p, sizeof(double) * (size_t)num_pairs, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(num_common, d_common.p, sizeof(int) * (size_t)num_pairs, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_view_selection_mvsnet(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                               const int32_t* obs_track, const uint8_t* view_estimated,
                                               const uint8_t* track_estimated, const double* cam_ext, const double* points,
                                               int32_t min_shared_tracks, int32_t num_neighbors, double theta0, double sigma1,
                                               double sigma2, int32_t column_window, int32_t* neighbor, double* score) {
  const Observations o{num_views, num_tracks, num_obs, obs_view, obs_track};
  int rc = check_observations(o);
  if (rc) return rc;
  if (num_neighbors < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_neighbors must not be negative");
  if (min_shared_tracks < 0 || column_window < 0)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative min_shared_tracks or column_window");
  if ((rc = check_score_parameters(theta0, sigma1, sigma2))) return rc;
  const size_t cells = (size_t)num_views * (size_t)num_neighbors;
  if ((num_views > 0 && (!cam_ext || (num_tracks > 0 && !points))) || (cells > 0 && (!neighbor || !score)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (num_views == 0) return 0;
  std::vector<int2> h_pairs;
  std::vector<double> h_score;
  if (num_obs > 0) {
    Plan plan;
    plan.build(o);
    if ((rc = ensure_device())) return rc;
    if ((rc = plan.upload()) || (rc = Plan::upload_flags(&plan.d_view_est, view_estimated, num_views)) ||
        (rc = Plan::upload_flags(&plan.d_track_est, track_estimated, num_tracks)) ||
        (rc = plan.d_cam.up(cam_ext, 6 * (size_t)num_views)) || (rc = plan.d_points.up(points, 4 * (size_t)num_tracks)))
      return rc;
    DevBuf<int2> d_pairs;
    DevBuf<int> d_shared, d_common;
    DevBuf<double> d_score;
    long long E = 0;
    if ((rc = run_graph(plan, num_views, min_shared_tracks, window_of(column_window), -1, &d_pairs, &d_shared, &E))) return rc;
    if (E > 0) {
      if ((rc = d_score.alloc((size_t)E)) || (rc = d_common.alloc((size_t)E))) return rc;
      if ((rc = run_scores(plan, E, d_pairs.p, nullptr, theta0, sigma1, sigma2, d_score.p, d_common.p))) return rc;
      HIP_TRY(hipDeviceSynchronize());
      h_pairs.resize((size_t)E);
      h_score.resize((size_t)E);
      HIP_TRY(hipMemcpy(h_pairs.data(), d_pairs.p, sizeof(int2) * (size_t)E, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(h_score.data(), d_score.p, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost));
    }
  }
  // the selection: every view's neighbours as (score, view), best first
  std::vector<long long> off((size_t)num_views + 1, 0);
  for (const int2& p : h_pairs) { ++off[p.x + 1]; ++off[p.y + 1]; }
  for (int v = 0; v < num_views; ++v) off[v + 1] += off[v];
  struct Item { double s; int v; };
  std::vector<Item> items(2 * h_pairs.size());
  {
    std::vector<long long> fill(off.begin(), off.end() - 1);
    for (size_t e = 0; e < h_pairs.size(); ++e) {
      items[fill[h_pairs[e].x]++] = Item{h_score[e], h_pairs[e].y};
      items[fill[h_pairs[e].y]++] = Item{h_score[e], h_pairs[e].x};
    }
  }
  const auto better = [](const Item& a, const Item& b) {
    const bool an = std::isnan(a.s), bn = std::isnan(b.s);
    if (an != bn) return bn;                      // a number before a NaN
    if (!an && a.s != b.s) return a.s > b.s;      // the larger score first
    return a.v < b.v;                             // equal scores, or two NaNs: the smaller view index
  };
  std::fill(neighbor, neighbor + cells, -1);
  std::fill(score, score + cells, 0.0);
  for (int v = 0; v < num_views; ++v) {
    Item* first = items.data() + off[v];
    Item* last = items.data() + off[v + 1];
    const long long keep = std::min<long long>(num_neighbors, last - first);
    std::partial_sort(first, first + keep, last, better);
    for (long long k = 0; k < keep; ++k) {
      neighbor[(size_t)v * num_neighbors + k] = first[k].v;
      score[(size_t)v * num_neighbors + k] = first[k].s;
    }
  }
  return 0;
}

extern "C" int theia_hip_find_common_tracks(int32_t num_views, int32_t num_tracks, int64_t num_obs, const int32_t* obs_view,
                                            const int32_t* obs_track, int32_t num_queries, const int64_t* offsets,
                                            const int32_t* views, int64_t track_capacity, int64_t* track_off, int32_t* tracks,
                                            int64_t* num_found) {
  const Observations o{num_views, num_tracks, num_obs, obs_view, obs_track};
  int rc = check_observations(o);
  if (rc) return rc;
  const int Q = num_queries;
  if (Q < 0 || track_capacity < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if ((Q > 0 && (!offsets || !views || !track_off || !num_found)) || (track_capacity > 0 && !tracks))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (Q == 0) return 0;
  if (offsets[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must start at 0");
  for (int q = 0; q < Q; ++q)
    if (offsets[q + 1] - offsets[q] < 2)   // CHECK_GT(views.size(), 1)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "query %d has fewer than 2 views", q);
  for (int64_t k = 0; k < offsets[Q]; ++k)
    if (views[k] < 0 || views[k] >= num_views)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "query entry %lld names a view out of range", (long long)k);
  if (num_obs == 0) {
    std::fill(track_off, track_off + Q + 1, (int64_t)0);
    *num_found = 0;
    return 0;
  }
  Plan plan;
  plan.build(o);
  if ((rc = ensure_device())) return rc;
  DevBuf<long long> d_q_off, d_out_off;
  DevBuf<int> d_q_views, d_count, d_tracks;
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
  if ((rc = plan.upload()) || (rc = d_q_off.up(offsets, (size_t)Q + 1)) || (rc = d_q_views.up(views, (size_t)offsets[Q])) ||
      (rc = d_count.alloc((size_t)Q)) || (rc = d_out_off.alloc((size_t)Q)))
    return rc;
  const int grid = grid_of((size_t)Q, kThreads / kTeam);
  k_common_tracks<false><<<grid, kThreads>>>(Q, d_q_off.p, d_q_views.p, plan.csr(), d_count.p, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  std::vector<int> count((size_t)Q);
  HIP_TRY(hipMemcpy(count.data(), d_count.p, sizeof(int) * (size_t)Q, hipMemcpyDeviceToHost));
  std::vector<long long> out_off((size_t)Q + 1, 0);
  for (int q = 0; q < Q; ++q) out_off[q + 1] = out_off[q] + count[q];
  const long long total = out_off[Q];
  const bool fits = total <= track_capacity;
  if (fits && total > 0) {
    if ((rc = d_tracks.alloc((size_t)total))) return rc;
    HIP_TRY(hipMemcpy(d_out_off.p, out_off.data(), sizeof(long long) * (size_t)Q, hipMemcpyHostToDevice));
    k_common_tracks<true><<<grid, kThreads>>>(Q, d_q_off.p, d_q_views.p, plan.csr(), nullptr, d_out_off.p, d_tracks.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(tracks, d_tracks.p, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost));
  }
  std::copy(out_off.begin(), out_off.end(), track_off);
  *num_found = total;
  return 0;
}
