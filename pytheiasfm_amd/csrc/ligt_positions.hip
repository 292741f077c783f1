// ligt_positions.hip -- LiGTPositionEstimator (global_pose_estimation/LiGT_position_estimator.cc:160-470; Cai et al.,
// "A Pose-only Solution to Visual Reconstruction and Navigation"): global positions from the global orientations and the
// tracks' normalised features alone, on the device in FP64.
//
// Per track of at least three observations the base pair (v1, v3) is the observation pair of largest
//   theta^2_ij = |[f_j]x R_j R_i' f_i|^2                                                   (GetBestBaseViews, :227-255)
// and every other observation (v2, f2) of the track gives one constraint B c_v1 + C c_v2 + D c_v3 = 0 on the camera
// positions (CalculateBCDForTrack, :257-289):
//   C = [f1]x R31 f3 a32' R_v2,   a32 = ([R32 f3]x f2)' [f2]x,   B = |[f2]x R32 f3|^2 [f1]x R_v1,   D = -(B + C)
// with R31 = R_v1 R_v3', R32 = R_v2 R_v3'.  The normal equations H = sum [B C D]' [B C D] on the 3 x 3 blocks of
// (v1, v2, v3), without the rows and columns of the held view (:94-121, :356-401), are a dense view-by-view matrix of
// the shape of the BA's reduced camera system; the positions are the eigenvector of H's smallest eigenvalue.
//
// Stages:
//   k_rotations   one thread per view: the rotation matrix, once
//   k_rays        one thread per observation: the world ray R_v' f.  R is orthonormal, so theta^2_ij = |ray_i x ray_j|^2
//                 up to rounding, and the pair search needs no matrix at all
//   k_base_pairs  one wavefront per track: the lanes stride over the len (len - 1) / 2 pairs in lexicographic (i, j)
//                 order, each keeps its first maximum, and the wave's arg-max takes the lowest pair index among equals
//                 (wave_reduce.h); base_pairs = observation indices within the track, -1 -1 = track skipped
//   plan (host)   after the 8-byte-per-track download: the view indexing in the reference's insertion order and, per
//                 3 x 3 block of H's lower triangle, the list of the items that feed it, in (track, observation) order
//   k_items       one thread per used track: B, C, D of every constraint in registers; B'B, B'D and D'D of a track all
//                 land on the (v1, v3) blocks and are summed within the track first -- three items per track, and three
//                 per constraint (C'C, B'C, C'D)
//   k_blocks      one thread per non-empty block: adds its items in order, writes the lower triangle (this, k_iterate and
//                 k_sign_vote: smallest_eigenvector.h, shared with linear_positions.hip)
//   k_shift       mu = kShiftMultiple n eps max diag H on the diagonal and x = b = 1 / sqrt(n) (spectral_shift.h: H's
//                 smallest eigenvalue is a rounding error of either sign on noise-free data; the shift moves no eigenvector)
//   dense_cholesky_factor once, then per inverse iteration dense_cholesky_solve_factored and k_iterate: normalise,
//                 |x_new - s x_old|_2 with s = sign(x_new . x_old), and the stop flag on the device (the pattern of
//                 lud_positions.hip: the host reads the flag once per chunk of iterations)
//   k_sign_vote   one launch over the view pairs (FlipSignOfPositionsIfNecessary, :432-470): integer votes, block sums,
//                 one integer atomic per workgroup
//
// Determinism: no floating-point atomics.  Every entry of H is a sum in (track, observation) order by one owner, every
// norm a fixed tree (block_sum), the votes are integers.  Two runs on one input are bit-identical.
#include "smallest_eigenvector.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kTracksPerBlock = kThreads / 64;   // k_base_pairs: one wavefront per track
// mu = kShiftMultiple * n * eps * max diag H (DESIGN.md 3.6f has the rule and the scenes it was chosen on)
constexpr double kShiftMultiple = 1.0;

__global__ __launch_bounds__(kThreads) void k_rays(int num_obs, const int* __restrict__ obs_view,
                                                   const double* __restrict__ feat, const double* __restrict__ R,
                                                   double* __restrict__ ray) {
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= num_obs) return;
  const double* r = R + 9 * (size_t)obs_view[o];
  const double x = feat[2 * (size_t)o], y = feat[2 * (size_t)o + 1];
#pragma unroll
  for (int c = 0; c < 3; ++c) ray[3 * (size_t)o + c] = (r[c] * x + r[3 + c] * y) + r[6 + c];
}

// first pair index of row i among the pairs (i, j > i) of L observations
__device__ __forceinline__ long long pair_row_start(long long i, long long L) { return i * (2 * L - i - 1) / 2; }

__global__ __launch_bounds__(kThreads) void k_base_pairs(int num_tracks, const int* __restrict__ off,
                                                         const double* __restrict__ ray, int2* __restrict__ base) {
  const int t = blockIdx.x * kTracksPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= num_tracks) return;   // wave-uniform
  const int o0 = off[t];
  const long long L = off[t + 1] - o0;
  if (L < 3) {
    if (lane == 0) base[t] = make_int2(-1, -1);
    return;
  }
  const long long P = L * (L - 1) / 2;
  double best = -1.0;        // no candidate: 0 and NaN never beat the reference's starting value 0 under `>`
  long long best_p = P;
  if (lane < P) {
    // decode this lane's first pair, then advance by 64 pairs per step
    long long p = lane;
    const double s = 2.0 * (double)L - 1.0;
    long long i = (long long)((s - sqrt(fmax(0.0, s * s - 8.0 * (double)p))) * 0.5);
    i = max(0LL, min(i, L - 2));
    while (i > 0 && pair_row_start(i, L) > p) --i;
    while (i < L - 2 && pair_row_start(i + 1, L) <= p) ++i;
    long long j = i + 1 + (p - pair_row_start(i, L));
    double th_best = 0.0;
    for (; p < P; p += 64) {
      const double* ri = ray + 3 * (size_t)(o0 + i);
      const double* rj = ray + 3 * (size_t)(o0 + j);
      double c[3];
      cross3(ri, rj, c);
      const double th = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
      if (th > th_best) { th_best = th; best = th; best_p = p; }
      j += 64;
      while (j >= L && i < L - 2) { ++i; j = j - L + i + 1; }
    }
  }
  const double m = wave_max_abs(best);   // -1.0 when no lane holds a positive theta^2
  // the lowest pair index among the lanes that hold the maximum: min p = ~max(~p), high word first
  const bool mine = m > 0.0 && best == m;
  const unsigned hi = mine ? ~(unsigned)((unsigned long long)best_p >> 32) : 0u;
  const unsigned hm = wave_max_u32(hi);
  const unsigned lo = (mine && hi == hm) ? ~(unsigned)((unsigned long long)best_p & 0xffffffffull) : 0u;
  const unsigned lm = wave_max_u32(lo);
  if (lane == 0) {
    if (!(m > 0.0)) {
      base[t] = make_int2(-1, -1);
    } else {
      const long long p = (long long)(((unsigned long long)(~hm) << 32) | (unsigned long long)(~lm));
      const double s = 2.0 * (double)L - 1.0;
      long long i = (long long)((s - sqrt(fmax(0.0, s * s - 8.0 * (double)p))) * 0.5);
      i = max(0LL, min(i, L - 2));
      while (i > 0 && pair_row_start(i, L) > p) --i;
      while (i < L - 2 && pair_row_start(i + 1, L) <= p) ++i;
      base[t] = make_int2((int)i, (int)(i + 1 + (p - pair_row_start(i, L))));
    }
  }
}

// One thread per used track.  Items of track t from item_base[t]: [0] sum B'B, [1] sum B'D, [2] sum D'D, then per
// constraint (every observation but the two of the base pair, in order) C'C, B'C, C'D.  The observation of v3 itself
// gives B = C = D = 0 in exact arithmetic and is no constraint here.
__global__ __launch_bounds__(kThreads) void k_items(int num_tracks, const int* __restrict__ off,
                                                    const int* __restrict__ obs_view, const double* __restrict__ feat,
                                                    const double* __restrict__ R, const double* __restrict__ ray,
                                                    const int2* __restrict__ base, const long long* __restrict__ item_base,
                                                    double* __restrict__ items) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= num_tracks) return;
  const long long ib = item_base[t];
  if (ib < 0) return;
  const int o0 = off[t], L = off[t + 1] - o0;
  const int bi = base[t].x, bj = base[t].y;
  const double f1[3] = {feat[2 * (size_t)(o0 + bi)], feat[2 * (size_t)(o0 + bi) + 1], 1.0};
  const double* R1 = R + 9 * (size_t)obs_view[o0 + bi];
  const double z3[3] = {ray[3 * (size_t)(o0 + bj)], ray[3 * (size_t)(o0 + bj) + 1], ray[3 * (size_t)(o0 + bj) + 2]};
  // u = [f1]x R31 f3 = f1 x (R1 z3),  M1 = [f1]x R1
  double g[3], u[3], M1[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) g[r] = (R1[3 * r] * z3[0] + R1[3 * r + 1] * z3[1]) + R1[3 * r + 2] * z3[2];
  cross3(f1, g, u);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double col[3] = {R1[c], R1[3 + c], R1[6 + c]};
    double m[3];
    cross3(f1, col, m);
    M1[c] = m[0]; M1[3 + c] = m[1]; M1[6 + c] = m[2];
  }
  double S11[9], S13[9], S33[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { S11[k] = 0.0; S13[k] = 0.0; S33[k] = 0.0; }
  double* out = items + 9 * (size_t)(ib + 3);
  for (int k = 0; k < L; ++k) {
    if (k == bi || k == bj) continue;
    const double f2[3] = {feat[2 * (size_t)(o0 + k)], feat[2 * (size_t)(o0 + k) + 1], 1.0};
    const double* R2 = R + 9 * (size_t)obs_view[o0 + k];
    double h[3], q[3], a32[3], w[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (R2[3 * r] * z3[0] + R2[3 * r + 1] * z3[1]) + R2[3 * r + 2] * z3[2];   // R32 f3
    cross3(h, f2, q);      // [R32 f3]x f2
    cross3(q, f2, a32);    // (q' [f2]x)'
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = (a32[0] * R2[c] + a32[1] * R2[3 + c]) + a32[2] * R2[6 + c];   // a32' R2
    cross3(f2, h, e);
    const double th = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    double B[9], Cm[9], D[9], T[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        B[3 * r + c] = th * M1[3 * r + c];
        Cm[3 * r + c] = u[r] * w[c];
        D[3 * r + c] = -(B[3 * r + c] + Cm[3 * r + c]);
      }
    atb(B, B, T);
#pragma unroll
    for (int q9 = 0; q9 < 9; ++q9) S11[q9] += T[q9];
    atb(B, D, T);
#pragma unroll
    for (int q9 = 0; q9 < 9; ++q9) S13[q9] += T[q9];
    atb(D, D, T);
#pragma unroll
    for (int q9 = 0; q9 < 9; ++q9) S33[q9] += T[q9];
    atb(Cm, Cm, T); store9(out, T);
    atb(B, Cm, T); store9(out + 9, T);
    atb(Cm, D, T); store9(out + 18, T);
    out += 27;
  }
  double* head = items + 9 * (size_t)ib;
  store9(head, S11); store9(head + 9, S13); store9(head + 18, S33);
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_ligt_positions(int32_t num_views, const double* orientations, int32_t num_tracks,
                                        const int32_t* track_offsets, const int32_t* obs_view, const double* obs_feature,
                                        int32_t num_edges, const int32_t* edges, const double* relative_translations,
                                        const theia_ligt_options* options, double* positions_out, uint8_t* estimated_out,
                                        int32_t* base_pairs_out, double* system_out, int32_t* system_index_out,
                                        theia_ligt_summary* summary) {
  const auto t_start = std::chrono::steady_clock::now();
  const int n = num_views, T = num_tracks, E = num_edges;
  theia_ligt_options o{1000, 0, 1e-8};
  if (options) o = *options;
  // ---- refusals, before the device is touched
  if (n < 1 || !orientations || !positions_out || !estimated_out || !summary)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no views, or a null output");
  if (T < 1 || !track_offsets || !obs_view || !obs_feature) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no tracks");
  if (E < 0 || (E > 0 && (!edges || !relative_translations)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view pairs without their arrays");
  if (o.max_power_iterations <= 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_power_iterations must be > 0");
  if (!(o.eigensolver_threshold > 0.0) || !std::isfinite(o.eigensolver_threshold))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "eigensolver_threshold must be positive and finite");
  if (track_offsets[0] < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets must start at >= 0");
  for (int t = 0; t < T; ++t)
    if (track_offsets[t + 1] < track_offsets[t])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track_offsets decrease at track %d", t);
  const int num_obs = track_offsets[T];
  {
    std::vector<int> seen(n, -1);
    bool any_long = false;
    for (int t = 0; t < T; ++t) {
      any_long |= track_offsets[t + 1] - track_offsets[t] >= 3;
      for (int k = track_offsets[t]; k < track_offsets[t + 1]; ++k) {
        const int v = obs_view[k];
        if (v < 0 || v >= n) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "observation %d names view %d of %d", k, v, n);
        if (seen[v] == t) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "track %d names view %d twice", t, v);
        seen[v] = t;
      }
    }
    for (int e = 0; e < 2 * E; ++e)
      if (edges[e] < 0 || edges[e] >= n)
        return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view pair %d names view %d of %d", e / 2, edges[e], n);
    if (!any_long) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no track with three observations: no track used");
  }

  int rc;
  if ((rc = thip::ensure_device())) return rc;
  theia_ligt_summary sm{};
  hipStream_t st = nullptr;
  DevBuf<double> d_aa, d_feat, d_R, d_ray;
  DevBuf<int> d_off, d_obs_view;
  DevBuf<int2> d_base;
  if ((rc = d_aa.up(orientations, 3 * (size_t)n)) || (rc = d_off.up(track_offsets, (size_t)T + 1)) ||
      (rc = d_obs_view.up(obs_view, num_obs)) || (rc = d_feat.up(obs_feature, 2 * (size_t)num_obs)) ||
      (rc = d_R.alloc(9 * (size_t)n)) || (rc = d_ray.alloc(3 * (size_t)num_obs)) || (rc = d_base.alloc(T)))
    return rc;

  // ---- set-up: rotations, rays, base pairs, plan
  k_rotations<kThreads><<<grid_of(n, kThreads), kThreads, 0, st>>>(n, d_aa.p, d_R.p);
  k_rays<<<grid_of(num_obs, kThreads), kThreads, 0, st>>>(num_obs, d_obs_view.p, d_feat.p, d_R.p, d_ray.p);
  k_base_pairs<<<grid_of(T, kTracksPerBlock), kThreads, 0, st>>>(T, d_off.p, d_ray.p, d_base.p);
  HIP_TRY(hipGetLastError());
  std::vector<int2> base(T);
  HIP_TRY(hipMemcpy(base.data(), d_base.p, sizeof(int2) * (size_t)T, hipMemcpyDeviceToHost));

  // the view indexing: v1, v2, v3 per constraint, constraints in (track, observation) order; the first view is held
  std::vector<int> idx(n, -2);
  std::vector<long long> item_base(T, -1);
  int m = 0;
  long long num_items = 0, num_constraints = 0;
  for (int t = 0; t < T; ++t) {
    const int o0 = track_offsets[t], L = track_offsets[t + 1] - o0;
    const int bi = base[t].x, bj = base[t].y;
    if (bi < 0) { sm.tracks_skipped += 1; continue; }
    if (L < 3 || bj <= bi || bj >= L) return set_error(THEIA_HIP_ERR_INTERNAL, "base pair of track %d out of range", t);
    sm.tracks_used += 1;
    const int v1 = obs_view[o0 + bi], v3 = obs_view[o0 + bj];
    for (int k = 0; k < L; ++k) {
      if (k == bi) continue;
      const int v2 = obs_view[o0 + k];
      if (idx[v1] == -2) idx[v1] = m++ - 1;
      if (idx[v2] == -2) idx[v2] = m++ - 1;
      if (idx[v3] == -2) idx[v3] = m++ - 1;
    }
    item_base[t] = num_items;
    num_items += 3 + 3 * (long long)(L - 2);
    num_constraints += L - 1;
  }
  if (sm.tracks_used == 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "no track has a pair of positive theta^2: no track used");
  if (num_items >= (1LL << 30)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "%lld 3 x 3 items: too many constraints", num_items);
  const int mf = m - 1;   // free views
  sm.num_views_in_system = m;
  sm.num_constraints = (int32_t)std::min<long long>(num_constraints, INT32_MAX);
  if (mf < 1) return set_error(THEIA_HIP_ERR_INTERNAL, "a used track with one view");

  SmallestEigenvector ev;
  if ((rc = ev.alloc(mf, system_out != nullptr))) return rc;

  // the segment list: per block (row >= col, free views) of the lower triangle its items, by a stable counting sort
  // an item (va, vb) holds X' Y with X on va and Y on vb: it lands on block (idx va, idx vb), transposed when that lies above
  BlockSegments seg;
  build_block_segments(mf, [&](auto&& emit) {
    for (int t = 0; t < T; ++t) {
      if (item_base[t] < 0) continue;
      const int o0 = track_offsets[t], L = track_offsets[t + 1] - o0;
      const int bi = base[t].x, bj = base[t].y;
      const int i1 = idx[obs_view[o0 + bi]], i3 = idx[obs_view[o0 + bj]];
      long long it = item_base[t];
      emit(i1, i1, it); emit(i1, i3, it + 1); emit(i3, i3, it + 2);
      it += 3;
      for (int k = 0; k < L; ++k) {
        if (k == bi || k == bj) continue;
        const int i2 = idx[obs_view[o0 + k]];
        emit(i2, i2, it); emit(i1, i2, it + 1); emit(i2, i3, it + 2);
        it += 3;
      }
    }
  }, &seg);

  DevBuf<double> d_items, d_rel;
  DevBuf<long long> d_item_base;
  DevBuf<int> d_idx;
  DevBuf<int2> d_edges;
  if ((rc = d_items.alloc(9 * (size_t)num_items)) || (rc = d_item_base.up(item_base.data(), T)) || (rc = d_idx.up(idx.data(), n)) ||
      (rc = d_edges.up(edges, E)) || (rc = d_rel.up(relative_translations, 3 * (size_t)E)) || (rc = ev.upload(seg, st)))
    return rc;
  HIP_TRY(hipStreamSynchronize(st));
  sm.setup_ms = ms_since(t_start);

  // ---- assembly
  const auto t_assemble = std::chrono::steady_clock::now();
  k_items<<<grid_of(T, kThreads), kThreads, 0, st>>>(T, d_off.p, d_obs_view.p, d_feat.p, d_R.p, d_ray.p, d_base.p,
                                                    d_item_base.p, d_items.p);
  if ((rc = ev.assemble(d_items.p, kShiftMultiple, st))) return rc;
  sm.assemble_ms = ms_since(t_assemble);

  if ((rc = ev.factor(st, &sm, summary))) return rc;

  // ---- inverse iteration, sign vote (FlipSignOfPositionsIfNecessary needs view pairs), scatter
  const auto t_eig = std::chrono::steady_clock::now();
  if ((rc = ev.iterate(o.max_power_iterations, o.eigensolver_threshold, st)) ||
      (E > 0 && (rc = ev.vote(E, d_edges.p, d_idx.p, d_R.p, d_rel.p, st))) || (rc = ev.fetch()))
    return rc;
  sm.eig_ms = ms_since(t_eig);
  ev.scatter(n, idx, positions_out, estimated_out, system_out, system_index_out, &sm);
  if (base_pairs_out)
    for (int t = 0; t < T; ++t) { base_pairs_out[2 * (size_t)t] = base[t].x; base_pairs_out[2 * (size_t)t + 1] = base[t].y; }
  *summary = sm;
  return 0;
}
