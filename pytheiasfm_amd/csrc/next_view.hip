// next_view.hip -- the two counting stages of the incremental estimator's inner loop:
//   theia_hip_visibility_scores: VisibilityPyramid (sfm/visibility_pyramid.cc:47-103) of every view, as FindViewsToLocalize
//     (sfm/incremental_reconstruction_estimator.cc:422-463) fills it: the view's observations of ESTIMATED tracks only.
//   theia_hip_set_underconstrained_unestimated: the estimators' SetUnderconstrainedAsUnestimated loop
//     (incremental_reconstruction_estimator.cc:612-620, global_reconstruction_estimator.cc:100-110) over
//     SetUnderconstrainedViewsToUnestimated / SetUnderconstrainedTracksToUnestimated (reconstruction_estimator_utils.cc:291-350).
//
// k_visibility   one workgroup of kThreads = 256 per view.  The finest level's occupancy is a bitmap in LDS, one bit per cell,
//                the cell (x, y) at its Morton index (x's bits even, y's odd): the four children of a cell of the next coarser
//                level are then four consecutive bits, and a level is derived from the finer one by OR-ing every nibble into
//                one bit (fold4 below).  4^levels bits: 256 words of 64 bits at seven levels, one per thread.  The lanes stride
//                over the view's observations and set bits with an LDS atomicOr; the number of estimated tracks is one wave
//                reduction per wave and an LDS sum.  Every thread adds popcount * weight of the words it derived, one
//                workgroup reduction gives the score.  Integers only, no global atomic: two calls give the same bytes.
//                A NaN or infinite coordinate raises *bad (a plain store of 1 by whoever sees one); the host reads it before it
//                writes any output.
// k_uc_count     one lane per observation: adds 1 to its view's counter when its track is estimated (view pass), or to its
//                track's counter when its view is estimated (track pass).  Integer atomics: the sums do not depend on order.
// k_uc_decide    one lane per view (track): clears the flag of an estimated item whose counter is under the minimum, counts the
//                cleared ones into the round's state, and zeroes the counter for the next round.
// The flags a pass reads are not the flags it writes, so the parallel pass equals the reference's sequential one.
#include "wave_reduce.h"
#include "device_util.h"

#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 7;                       // 16^8 = 2^32 overflows the reference's int score at eight
constexpr int kMaxWords = (1 << (2 * kMaxLevels)) / 64;   // 256 words of the finest level at seven levels
// every level's words behind one another, finest first: 256 + 64 + 16 + 4 + 1 + 1 + 1
constexpr int kPyramidWords = kMaxWords + 64 + 16 + 4 + 1 + 1 + 1;
static_assert(kMaxWords <= kThreads, "one word of the finest level per thread");

// the 7 low bits of v to the even positions
__device__ __forceinline__ unsigned spread_bits(unsigned v) {
  v = (v | (v << 4)) & 0x0F0Fu;
  v = (v | (v << 2)) & 0x3333u;
  v = (v | (v << 1)) & 0x5555u;
  return v;
}

// bit k of the result = OR of the bits 4k .. 4k+3 of w, k < 16
__device__ __forceinline__ unsigned long long fold4(unsigned long long w) {
  w |= w >> 1;
  w |= w >> 2;
  w &= 0x1111111111111111ull;
  w = (w | (w >> 3)) & 0x0303030303030303ull;
  w = (w | (w >> 6)) & 0x000F000F000F000Full;
  w = (w | (w >> 12)) & 0x000000FF000000FFull;
  w = (w | (w >> 24)) & 0xFFFFull;
  return w;
}

// clamp((int)(C * x / extent), 0, C - 1) (visibility_pyramid.cc:71-78), the clamp taken in double so that the truncation is
// defined for every finite x; the product first, then the division
__device__ __forceinline__ int finest_cell(double x, int cells, int extent) {
  const double q = (double)cells * x / (double)extent;
  if (!(q > 0.0)) return 0;
  if (q >= (double)cells) return cells - 1;
  return (int)q;
}

__device__ __forceinline__ int words_of_level(int level) {   // level = number of doublings: 4^level cells
  const int bits = 1 << (2 * level);
  return bits >= 64 ? bits / 64 : 1;
}

__global__ __launch_bounds__(kThreads) void k_visibility(const long long* __restrict__ obs_off, const double2* __restrict__ obs_uv,
                                                         const int* __restrict__ obs_track,
                                                         const uint8_t* __restrict__ track_estimated,
                                                         const int2* __restrict__ image_size, int levels,
                                                         int* __restrict__ num_estimated, int* __restrict__ score,
                                                         int* __restrict__ bad) {
  __shared__ unsigned long long pyr[kPyramidWords];
  __shared__ int wave_count[kThreads / 64], wave_score[kThreads / 64];
  const int v = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < kPyramidWords; k += kThreads) pyr[k] = 0ull;
  __syncthreads();

  const int2 wh = image_size[v];
  const int cells = 1 << levels;
  int n_est = 0;
  bool nonfinite = false;
  for (long long k = obs_off[v] + tid, end = obs_off[v + 1]; k < end; k += kThreads) {
    const double2 p = obs_uv[k];
    nonfinite |= !(isfinite(p.x) && isfinite(p.y));
    if (!track_estimated[obs_track[k]]) continue;
    ++n_est;
    const unsigned idx = spread_bits((unsigned)finest_cell(p.x, cells, wh.x)) | (spread_bits((unsigned)finest_cell(p.y, cells, wh.y)) << 1);
    atomicOr(&pyr[idx >> 6], 1ull << (idx & 63u));
  }
  if (nonfinite) *bad = 1;
  __syncthreads();

  // level l has 4^l cells (l = levels: the finest; l = 1: the reference's level 0, a 2 x 2 grid, weight 4)
  int part = 0, base = 0;
  for (int l = levels; l >= 1; --l) {
    const int nw = words_of_level(l);
    if (tid < nw) part += __popcll(pyr[base + tid]) << (2 * l);
    if (l > 1) {
      const int cw = words_of_level(l - 1);
      if (tid < cw) {
        unsigned long long w = 0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * tid + q < nw) w |= fold4(pyr[base + 4 * tid + q]) << (16 * q);
        pyr[base + nw + tid] = w;
      }
      __syncthreads();
    }
    base += nw;
  }

  // both sums over the workgroup: a wave reduction each, then the four waves through LDS
  const int wave = tid >> 6;
  part = wave_sum_butterfly(part);
  n_est = wave_sum_butterfly(n_est);
  if ((tid & 63) == 0) { wave_count[wave] = n_est; wave_score[wave] = part; }
  __syncthreads();
  if (tid == 0) {
    int n = 0, s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { n += wave_count[w]; s += wave_score[w]; }
    num_estimated[v] = n;
    score[v] = s;
  }
}

struct SweepRound { int views_removed, tracks_removed; };

// view_pass: count[view] += track_estimated[track]; else count[track] += view_estimated[view]
__global__ __launch_bounds__(kThreads) void k_uc_count(long long num_obs, const int* __restrict__ obs_view,
                                                       const int* __restrict__ obs_track,
                                                       const uint8_t* __restrict__ view_estimated,
                                                       const uint8_t* __restrict__ track_estimated, int view_pass,
                                                       int* __restrict__ count) {
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= num_obs) return;
  const int v = obs_view[k], t = obs_track[k];
  if (view_pass) {
    if (track_estimated[t]) atomicAdd(&count[v], 1);
  } else {
    if (view_estimated[v]) atomicAdd(&count[t], 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_uc_decide(int n, int minimum, uint8_t* __restrict__ estimated,
                                                        int* __restrict__ count, int* __restrict__ removed) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  int gone = 0;
  if (i < n) {
    if (estimated[i] && count[i] < minimum) { estimated[i] = 0; gone = 1; }
    count[i] = 0;
  }
  gone = wave_sum_butterfly(gone);
  if ((threadIdx.x & 63) == 0 && gone) atomicAdd(removed, gone);
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_visibility_scores(int32_t num_views, const int64_t* obs_off, const double* obs_uv,
                                           const int32_t* obs_track, int32_t num_tracks, const uint8_t* track_estimated,
                                           const int32_t* image_size, int32_t num_pyramid_levels,
                                           int32_t* num_estimated_tracks, int32_t* score) {
  if (num_views < 0 || num_tracks < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if (num_pyramid_levels < 1 || num_pyramid_levels > kMaxLevels)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_pyramid_levels %d outside 1..%d", (int)num_pyramid_levels, kMaxLevels);
  if (num_views == 0) return 0;
  if (!obs_off || !obs_uv || !obs_track || !track_estimated || !image_size || !num_estimated_tracks || !score)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (obs_off[0] < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "obs_off starts below 0");
  for (int v = 0; v < num_views; ++v) {
    if (obs_off[v + 1] < obs_off[v]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "obs_off decreases at view %d", v);
    if (image_size[2 * v] <= 0 || image_size[2 * v + 1] <= 0)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view %d: image size %d x %d (the reference CHECKs > 0)", v,
                       (int)image_size[2 * v], (int)image_size[2 * v + 1]);
  }
  const int64_t total = obs_off[num_views];
  for (int64_t k = obs_off[0]; k < total; ++k)
    if (obs_track[k] < 0 || obs_track[k] >= num_tracks)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld: track %d out of range", (long long)k, (int)obs_track[k]);

  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<long long> d_off;
  DevBuf<double2> d_uv;
  DevBuf<int> d_track, d_n, d_score, d_bad;
  DevBuf<int2> d_size;
  DevBuf<uint8_t> d_est;
  if ((rc = d_off.up(obs_off, (size_t)num_views + 1)) || (rc = d_uv.up(obs_uv, (size_t)total)) ||
      (rc = d_track.up(obs_track, (size_t)total)) || (rc = d_est.up(track_estimated, (size_t)num_tracks)) ||
      (rc = d_size.up(image_size, (size_t)num_views)) || (rc = d_n.alloc(num_views)) || (rc = d_score.alloc(num_views)) ||
      (rc = d_bad.alloc(1)))
    return rc;
  HIP_TRY(hipMemset(d_bad.p, 0, sizeof(int)));
  k_visibility<<<num_views, kThreads>>>(d_off.p, d_uv.p, d_track.p, d_est.p, d_size.p, num_pyramid_levels, d_n.p, d_score.p,
                                        d_bad.p);
  HIP_TRY(hipGetLastError());
  int h_bad = 0;
  HIP_TRY(hipMemcpy(&h_bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost));
  if (h_bad) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a NaN or infinite coordinate in obs_uv");
  HIP_TRY(hipMemcpy(num_estimated_tracks, d_n.p, sizeof(int) * (size_t)num_views, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(score, d_score.p, sizeof(int) * (size_t)num_views, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_set_underconstrained_unestimated(int32_t num_views, int32_t num_tracks, int64_t num_obs,
                                                          const int32_t* obs_view, const int32_t* obs_track,
                                                          uint8_t* view_estimated, uint8_t* track_estimated,
                                                          int32_t* views_removed, int32_t* tracks_removed, int32_t* rounds) {
  constexpr int kMinNumTracks = 3, kMinNumViews = 2;   // reconstruction_estimator_utils.cc:323, :292
  if (num_views < 0 || num_tracks < 0 || num_obs < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "negative count");
  if ((num_obs > 0 && (!obs_view || !obs_track)) || (num_views > 0 && !view_estimated) || (num_tracks > 0 && !track_estimated))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  for (int64_t k = 0; k < num_obs; ++k)
    if (obs_view[k] < 0 || obs_view[k] >= num_views || obs_track[k] < 0 || obs_track[k] >= num_tracks)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %lld: (view %d, track %d) out of range", (long long)k,
                       (int)obs_view[k], (int)obs_track[k]);
  // (without views and tracks the reference's loop makes its one round and removes nothing)
  int total_views = 0, total_tracks = 0, num_rounds = 1;
  if (num_views > 0 || num_tracks > 0) {
    num_rounds = 0;
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<int> d_view, d_track, d_cnt_view, d_cnt_track;
    DevBuf<uint8_t> d_vest, d_test;
    DevBuf<SweepRound> d_round;
    if ((rc = d_view.up(obs_view, (size_t)num_obs)) || (rc = d_track.up(obs_track, (size_t)num_obs)) ||
        (rc = d_vest.up(view_estimated, num_views)) || (rc = d_test.up(track_estimated, num_tracks)) ||
        (rc = d_cnt_view.alloc(num_views)) || (rc = d_cnt_track.alloc(num_tracks)) || (rc = d_round.alloc(1)))
      return rc;
    HIP_TRY(hipMemset(d_cnt_view.p, 0, sizeof(int) * (size_t)std::max(1, (int)num_views)));
    HIP_TRY(hipMemset(d_cnt_track.p, 0, sizeof(int) * (size_t)std::max(1, (int)num_tracks)));
    // :613-620, as written: `&&`, so the loop ends as soon as EITHER pass removed nothing.  Two integers come back per round.
    SweepRound r{-1, -1};
    while (r.views_removed != 0 && r.tracks_removed != 0) {
      HIP_TRY(hipMemset(d_round.p, 0, sizeof(SweepRound)));
      if (num_obs > 0)
        k_uc_count<<<grid_of((size_t)num_obs, kThreads), kThreads>>>(num_obs, d_view.p, d_track.p, d_vest.p, d_test.p, 1, d_cnt_view.p);
      if (num_views > 0)
        k_uc_decide<<<grid_of(num_views, kThreads), kThreads>>>(num_views, kMinNumTracks, d_vest.p, d_cnt_view.p, &d_round.p->views_removed);
      if (num_obs > 0)
        k_uc_count<<<grid_of((size_t)num_obs, kThreads), kThreads>>>(num_obs, d_view.p, d_track.p, d_vest.p, d_test.p, 0, d_cnt_track.p);
      if (num_tracks > 0)
        k_uc_decide<<<grid_of(num_tracks, kThreads), kThreads>>>(num_tracks, kMinNumViews, d_test.p, d_cnt_track.p, &d_round.p->tracks_removed);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(&r, d_round.p, sizeof(SweepRound), hipMemcpyDeviceToHost));
      total_views += r.views_removed;
      total_tracks += r.tracks_removed;
      ++num_rounds;
    }
    if (num_views > 0) HIP_TRY(hipMemcpy(view_estimated, d_vest.p, (size_t)num_views, hipMemcpyDeviceToHost));
    if (num_tracks > 0) HIP_TRY(hipMemcpy(track_estimated, d_test.p, (size_t)num_tracks, hipMemcpyDeviceToHost));
  }
  if (views_removed) *views_removed = total_views;
  if (tracks_removed) *tracks_removed = total_tracks;
  if (rounds) *rounds = num_rounds;
  return 0;
}
