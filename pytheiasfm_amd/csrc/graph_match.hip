// graph_match.hip -- the image-pair selection in front of the matcher: FisherVectorExtractor::ExtractGlobalDescriptor
// (matching/fisher_vector_extractor.cc:56-69, the element-wise mean in this fork) and GraphMatch (matching/graph_match.cc:48-130)
// as FeatureExtractorAndMatcher::SelectImagePairsWithGlobalDescriptorMatching drives them (sfm/feature_extractor_and_matcher.cc:
// 356-381).  The rule, its closed form, the pinned arithmetic and the stated deviations are in include/theia_hip.h and DESIGN.md
// 3.6p.
//
// The fact the design rests on: the reference's loop is sequential in i, but what it selects has a closed form over the kNN
// lists alone.  With kNN(x) the k nearest images of x under (distance, index) and inv(x) = { y : x in kNN(y) }, row a of the
// result (the pairs (a, i), a < i) is
//   for s in kNN(a):  s itself if s > a, and every i in inv(s) with i > a
//   for s in inv(a):  s itself if s > a, and every i in inv(s) with i > a and i > s
// so one workgroup owns one row, sets bits in LDS and writes the row once.
//
//   k_gd_pool       one lane per (image, dimension): the float sum over the image's features in order, divided once
//   k_gd_transpose  the global descriptors as [dim][N], so that lanes over the candidates read consecutive floats
//   k_gd_knn        one workgroup per group of 8 queries, their descriptors held once in LDS, lanes over the candidates:
//                   d = fmaf chain over the dimensions of (q - c)^2, key = (bits(d) << 32) | candidate, a row of keys per
//                   query in a workspace; the k smallest by a radix select of the k-th key, then a workgroup-wide bitonic
//                   sort of those k in LDS (of the whole row where k is no small part of it), written ascending
//   k_gm_count + DeviceScan::ExclusiveSum + k_gm_fill   the inverse lists as a CSR (their inner order is free: only membership
//                   is read)
//   k_gm_rows       the two loops above, one wave per s, lanes over inv(s); the row's bits and its two counts
//   DeviceScan::ExclusiveSum over the row counts, k_gm_emit   the pairs in ascending (image1, image2)
// Every output is a minimum, an integer or a set: the same bytes on every run.
#include "device_util.h"

#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQueries = 8;           // queries a workgroup of k_gd_knn takes at a time
constexpr int kQueryChunk = 1024;     // dimensions of their descriptors held in LDS at a time (32 KB)
constexpr int kSelKeys = 1024;        // the selected keys of a row in LDS (8 KB): the select route takes k up to this
constexpr int kMaxKnnGroups = 768;    // workgroups of k_gd_knn (three per CU fit by LDS): each walks the groups of queries
                                      // blockIdx.x, + gridDim.x, ...
constexpr int kBatch = 8;             // keys a lane loads from a workspace row before it uses the first
constexpr size_t kMaxRowBytes = 64 * 1024;   // the two bit rows of k_gm_rows in LDS

typedef unsigned long long ull;

__global__ __launch_bounds__(kThreads) void k_gd_pool(int num_images, int dim, const int64_t* __restrict__ feat_off,
                                                      const float* __restrict__ desc, float* __restrict__ out,
                                                      int* __restrict__ nan_flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (int64_t)num_images * dim) return;
  const int img = (int)(t / dim), d = (int)(t - (int64_t)img * dim);
  const int64_t begin = feat_off[img], end = feat_off[img + 1];   // end > begin: checked on the host
  float acc = 0.0f;
  bool nan = false;
  for (int64_t f = begin; f < end; ++f) {   // the pinned order: one chain, never split
    const float x = desc[f * dim + d];
    nan |= x != x;
    acc += x;
  }
  out[t] = acc / (float)(end - begin);      // IEEE division (the compiler's default for float / float in device code)
  if (nan) *nan_flag = 1;                   // every writer stores the same value
}

__global__ __launch_bounds__(kThreads) void k_gd_transpose(int N, int dim, const float* __restrict__ G, float* __restrict__ GT) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (int64_t)N * dim) return;
  const int d = (int)(t / N), j = (int)(t - (int64_t)d * N);
  GT[t] = G[(int64_t)j * dim + d];
}

__device__ __forceinline__ void compare_exchange(uint64_t* a, int lo, int hi) {
  const uint64_t x = a[lo], y = a[hi];
  if (y < x) { a[lo] = y; a[hi] = x; }
}

// a[0 .. n) ascending, by the whole workgroup.  The bitonic network in the form whose every comparator puts the smaller value at
// the lower index (each merge opens with the mirrored step), over the next power of two: elements at n and beyond would be
// +infinity, no comparator moves one, so those that touch them are skipped and any n sorts in place.  Ends with a barrier.
__device__ void sort_ascending(uint64_t* a, int n) {
  int P = 1;
  while (P < n) P <<= 1;
  const int half = P >> 1;
  for (int size = 2; size <= P; size <<= 1) {
    const int hs = size >> 1;
    for (int t = threadIdx.x; t < half; t += kThreads) {
      const int o = t & (hs - 1), base = (t - o) << 1;
      const int hi = base + size - 1 - o;
      if (hi < n) compare_exchange(a, base + o, hi);
    }
    __syncthreads();
    for (int stride = hs >> 1; stride >= 1; stride >>= 1) {
      for (int t = threadIdx.x; t < half; t += kThreads) {
        const int o = t & (stride - 1), lo = ((t - o) << 1) + o;
        if (lo + stride < n) compare_exchange(a, lo, lo + stride);
      }
      __syncthreads();
    }
  }
}

// The k-th smallest (k >= 1) of the n distinct keys a[0 .. n), by the whole workgroup: a radix select from the top byte down,
// one 256-bin histogram in LDS per byte; the bytes of the index part that n - 1 does not reach are zero in every key and are
// skipped.  hist [256] and pick [2] are LDS.  Ends with a barrier.
__device__ uint64_t select_kth(const uint64_t* a, int n, int k, unsigned* hist, unsigned* pick) {
  uint64_t prefix = 0, mask = 0;
  unsigned remaining = (unsigned)k;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (shift < 32 && shift > 0 && ((uint32_t)(n - 1) >> shift) == 0) { mask |= 255ull << shift; continue; }
    hist[threadIdx.x] = 0;   // kThreads == 256 bins
    __syncthreads();
    for (int j0 = threadIdx.x; j0 < n; j0 += kThreads * kBatch) {
      uint64_t key[kBatch];   // the loads of a batch are in flight together: a row in the workspace is L2's, not LDS's
#pragma unroll
      for (int u = 0; u < kBatch; ++u) key[u] = j0 + u * kThreads < n ? a[j0 + u * kThreads] : 0;
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (j0 + u * kThreads < n && (key[u] & mask) == prefix) atomicAdd(hist + (unsigned)((key[u] >> shift) & 255), 1u);
    }
    __syncthreads();
    if (wave == 0) {   // the bin that holds rank `remaining`: four bins per lane, a wave scan over the lanes' sums
      unsigned h[4], sum = 0;
      for (int b = 0; b < 4; ++b) { h[b] = hist[4 * lane + b]; sum += h[b]; }
      unsigned incl = sum;
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      unsigned before = incl - sum;
      if (before < remaining && remaining <= incl) {   // exactly one lane
        int b = 0;
        while (before + h[b] < remaining) before += h[b++];
        pick[0] = 4 * lane + b;
        pick[1] = before;
      }
    }
    __syncthreads();
    prefix |= (uint64_t)pick[0] << shift;
    mask |= 255ull << shift;
    remaining -= pick[1];
    __syncthreads();   // pick and hist are written again in the next pass
  }
  return prefix;
}

// G [N][dim], GT [dim][N].  knn_key [N][k]: the k smallest keys of every query, ascending.  workspace [gridDim.x][kQueries][N]
// keys.  A workgroup takes kQueries consecutive queries at a time, so that every candidate value it loads serves all of them
// (one query per pass would read the whole of GT once per query: 51 GB at 10 000 images of dim 128); a lane keeps one chain per
// query, each in the pinned order.  Then row by row: the keys are distinct, so the k smallest are one set however they are
// found; where k is small against the row (select == true: 2 k <= N and k <= kSelKeys) the k-th smallest key is selected, the
// keys up to it are gathered in LDS (in any order) and those k are sorted; else the whole row is sorted where it lies.
__global__ __launch_bounds__(kThreads) void k_gd_knn(int N, int dim, int k, bool select, const float* __restrict__ G,
                                                     const float* __restrict__ GT, uint64_t* __restrict__ workspace,
                                                     uint64_t* __restrict__ knn_key) {
  __shared__ float q[kQueryChunk][kQueries];
  __shared__ uint64_t sel[kSelKeys];
  __shared__ unsigned hist[256], pick[2], sel_count;
  uint64_t* rows = workspace + (size_t)blockIdx.x * kQueries * (size_t)N;
  for (int i0 = blockIdx.x * kQueries; i0 < N; i0 += gridDim.x * kQueries) {
    const int nq = min(kQueries, N - i0);
    for (int jb = 0; jb < N; jb += kThreads) {
      const int j = jb + (int)threadIdx.x;
      float acc[kQueries];
#pragma unroll
      for (int u = 0; u < kQueries; ++u) acc[u] = 0.0f;
      for (int c0 = 0; c0 < dim; c0 += kQueryChunk) {
        const int cn = min(kQueryChunk, dim - c0);
        if (dim > kQueryChunk || jb == 0) {   // the same for every lane; descriptors of one chunk are loaded once per group
          __syncthreads();
          for (int t = threadIdx.x; t < cn * kQueries; t += kThreads) {
            const int d = t / kQueries, u = t % kQueries;
            q[d][u] = u < nq ? G[(size_t)(i0 + u) * dim + c0 + d] : 0.0f;
          }
          __syncthreads();
        }
        if (j < N)
#pragma unroll 8
          for (int d = 0; d < cn; ++d) {   // unrolled: eight independent loads in flight per lane
            const float c = GT[(size_t)(c0 + d) * N + j];
#pragma unroll
            for (int u = 0; u < kQueries; ++u) {
              const float diff = q[d][u] - c;
              acc[u] = __fmaf_rn(diff, diff, acc[u]);
            }
          }
      }
      // acc >= +0 and no NaN (finite inputs: checked on the host), so the unsigned order of the key is (distance, index)
      if (j < N) {
#pragma unroll
        for (int u = 0; u < kQueries; ++u)
          if (u < nq) rows[(size_t)u * N + j] = j == i0 + u ? ~0ull : ((uint64_t)__float_as_uint(acc[u]) << 32 | (uint32_t)j);
      }
    }
    __syncthreads();
    for (int u = 0; u < nq; ++u) {
      uint64_t* keys = rows + (size_t)u * N;
      if (threadIdx.x == 0) sel_count = 0;
      __syncthreads();
      // the query's own entry is the largest key there is: k <= N - 1 never reaches it
      if (select) {
        const uint64_t kth = select_kth(keys, N, k, hist, pick);
        for (int j0 = threadIdx.x; j0 < N; j0 += kThreads * kBatch) {
          uint64_t key[kBatch];
#pragma unroll
          for (int b = 0; b < kBatch; ++b) key[b] = j0 + b * kThreads < N ? keys[j0 + b * kThreads] : ~0ull;   // > kth
#pragma unroll
          for (int b = 0; b < kBatch; ++b)
            if (key[b] <= kth) {   // exactly k keys, in any order
              const unsigned at = atomicAdd(&sel_count, 1u);
              if (at < (unsigned)k) sel[at] = key[b];   // k <= kSelKeys; the test only keeps a wrong count inside the array
            }
        }
        __syncthreads();
        sort_ascending(sel, k);
      } else {
        sort_ascending(keys, N);
      }
      const uint64_t* sorted = select ? sel : keys;
      for (int s = threadIdx.x; s < k; s += kThreads) knn_key[(size_t)(i0 + u) * k + s] = sorted[s];
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_gm_count(int64_t total, const uint64_t* __restrict__ knn_key, ull* __restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t < total) atomicAdd(count + (uint32_t)knn_key[t], 1ull);
}

__global__ __launch_bounds__(kThreads) void k_gm_fill(int64_t total, int k, const uint64_t* __restrict__ knn_key,
                                                      ull* __restrict__ cursor, int32_t* __restrict__ inv) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t < total) inv[atomicAdd(cursor + (uint32_t)knn_key[t], 1ull)] = (int32_t)(t / k);
}

__device__ __forceinline__ void set_bit(uint32_t* row, int i) { atomicOr(row + (i >> 5), 1u << (i & 31)); }

// Row a of the selection.  LDS: all [W] | ranked [W] words.  matrix [N][W]; row_pairs / row_ranked [N].
__global__ __launch_bounds__(kThreads) void k_gm_rows(int N, int k, int W, const uint64_t* __restrict__ knn_key,
                                                      const ull* __restrict__ inv_off, const int32_t* __restrict__ inv,
                                                      uint32_t* __restrict__ matrix, ull* __restrict__ row_pairs,
                                                      ull* __restrict__ row_ranked) {
  extern __shared__ uint32_t gm_bits[];
  __shared__ unsigned partial[2][kWaves];
  uint32_t* all = gm_bits;
  uint32_t* ranked = gm_bits + W;
  const int a = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int w = threadIdx.x; w < 2 * W; w += kThreads) gm_bits[w] = 0;
  __syncthreads();
  // s in kNN(a): s, and every image that has s among its nearest
  for (int si = wave; si < k; si += kWaves) {
    const int s = (int)(uint32_t)knn_key[(size_t)a * k + si];
    if (lane == 0 && s > a) { set_bit(all, s); set_bit(ranked, s); }
    for (ull p = inv_off[s] + lane, end = inv_off[s + 1]; p < end; p += 64) {
      const int i = inv[p];
      if (i > a) set_bit(all, i);
    }
  }
  // s in inv(a): s, and every LATER image that has s among its nearest (an earlier one's entry is the one the reference drops)
  for (ull p0 = inv_off[a] + wave, end0 = inv_off[a + 1]; p0 < end0; p0 += kWaves) {
    const int s = inv[p0];
    if (lane == 0 && s > a) { set_bit(all, s); set_bit(ranked, s); }
    for (ull p = inv_off[s] + lane, end = inv_off[s + 1]; p < end; p += 64) {
      const int i = inv[p];
      if (i > a && i > s) set_bit(all, i);
    }
  }
  __syncthreads();
  unsigned n_all = 0, n_ranked = 0;
  for (int w = threadIdx.x; w < W; w += kThreads) {
    matrix[(size_t)a * W + w] = all[w];
    n_all += __popc(all[w]);
    n_ranked += __popc(ranked[w]);
  }
  for (int o = 32; o >= 1; o >>= 1) { n_all += __shfl_down(n_all, o); n_ranked += __shfl_down(n_ranked, o); }
  if (lane == 0) { partial[0][wave] = n_all; partial[1][wave] = n_ranked; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ull s_all = 0, s_ranked = 0;
    for (int w = 0; w < kWaves; ++w) { s_all += partial[0][w]; s_ranked += partial[1][w]; }
    row_pairs[a] = s_all;
    row_ranked[a] = s_ranked;
  }
}

// one wave per row: the set bits of row a, ascending, from row_off[a]
__global__ __launch_bounds__(64) void k_gm_emit(int W, const uint32_t* __restrict__ matrix, const ull* __restrict__ row_off,
                                                int32_t* __restrict__ pair1, int32_t* __restrict__ pair2) {
  const int a = blockIdx.x, lane = threadIdx.x;
  ull base = row_off[a];
  for (int w0 = 0; w0 < W; w0 += 64) {
    const int w = w0 + lane;
    uint32_t word = w < W ? matrix[(size_t)a * W + w] : 0u;
    const unsigned c = __popc(word);
    unsigned incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    ull pos = base + incl - c;
    while (word) {
      const int b = __ffs(word) - 1;
      word &= word - 1;
      pair1[pos] = a;
      pair2[pos] = w * 32 + b;
      ++pos;
    }
    base += __shfl(incl, 63);
  }
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" int theia_hip_mean_pool_descriptors(int32_t num_images, const int64_t* feat_off, int32_t dim, const float* descriptors,
                                               float* global_descriptors) {
  if (num_images < 0 || dim < 1) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad sizes");
  if (num_images == 0) return 0;
  if (!feat_off || !descriptors || !global_descriptors) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (feat_off[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "feat_off must start at 0");
  for (int i = 0; i < num_images; ++i) {
    if (feat_off[i + 1] < feat_off[i]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "feat_off must be non-decreasing");
    if (feat_off[i + 1] == feat_off[i])   // fisher_vector_extractor.cc:58
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "image %d has no features", i);
  }
  const int64_t out_count = (int64_t)num_images * dim;
  if (out_count > INT_MAX) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "2^31 or more global descriptor entries");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf<int64_t> d_feat_off;
  DevBuf<float> d_desc, d_out;
  DevBuf<int> d_flag;
  if ((rc = d_feat_off.up(feat_off, (size_t)num_images + 1)) ||
      (rc = d_desc.up(descriptors, (size_t)feat_off[num_images] * (size_t)dim)) || (rc = d_out.alloc((size_t)out_count)) ||
      (rc = d_flag.alloc(1)))
    return rc;
  HIP_TRY(hipMemset(d_flag.p, 0, sizeof(int)));
  k_gd_pool<<<grid_of((size_t)out_count, kThreads), kThreads, 0, nullptr>>>(num_images, dim, d_feat_off.p, d_desc.p, d_out.p, d_flag.p);
  HIP_TRY(hipGetLastError());
  int flag = 0;
  HIP_TRY(hipMemcpy(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a descriptor holds a NaN");   // fisher_vector_extractor.cc:64
  HIP_TRY(hipMemcpy(global_descriptors, d_out.p, sizeof(float) * (size_t)out_count, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int theia_hip_graph_match(int32_t num_images, int32_t dim, const float* global_descriptors,
                                     int32_t num_nearest_neighbors, int64_t pair_capacity, int32_t* pair_image1,
                                     int32_t* pair_image2, int64_t* num_pairs, int32_t* knn_index, float* knn_distance,
                                     theia_graph_match_stats* stats) {
  if (num_images < 0 || dim < 1 || pair_capacity < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad sizes");
  if (num_nearest_neighbors < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "num_nearest_neighbors must not be negative");
  if (!num_pairs || (num_images && !global_descriptors) || (pair_capacity && (!pair_image1 || !pair_image2)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int N = num_images, k = std::min(std::max(N - 1, 0), num_nearest_neighbors);   // graph_match.cc:56-58
  const int64_t entries = (int64_t)N * dim;
  if (entries > INT_MAX) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "2^31 or more global descriptor entries");
  for (int64_t t = 0; t < entries; ++t)
    if (!std::isfinite(global_descriptors[t]))   // a NaN distance has no place in the order
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "global descriptor %lld is not finite", (long long)(t / dim));
  theia_graph_match_stats S{};
  S.num_nearest_neighbors = k;
  if (N <= 1 || k == 0) {   // the reference's loops do not run
    *num_pairs = 0;
    if (stats) *stats = S;
    return 0;
  }
  const int W = (N + 31) / 32;
  if (2 * sizeof(uint32_t) * (size_t)W > kMaxRowBytes)
    return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "a row of %d bits does not fit the workgroup's memory", N);
  int rc = ensure_device();
  if (rc) return rc;

  // the k nearest of every image
  const size_t total = (size_t)N * (size_t)k;
  DevBuf<float> d_G, d_GT;
  DevBuf<uint64_t> d_knn, d_workspace;
  if ((rc = d_G.up(global_descriptors, (size_t)entries)) || (rc = d_GT.alloc((size_t)entries)) || (rc = d_knn.alloc(total))) return rc;
  k_gd_transpose<<<grid_of((size_t)entries, kThreads), kThreads, 0, nullptr>>>(N, dim, d_G.p, d_GT.p);
  const int groups = std::min((N + kQueries - 1) / kQueries, kMaxKnnGroups);
  const bool select = k <= kSelKeys && 2 * (int64_t)k <= N;
  if ((rc = d_workspace.alloc((size_t)groups * kQueries * (size_t)N))) return rc;
  k_gd_knn<<<groups, kThreads, 0, nullptr>>>(N, dim, k, select, d_G.p, d_GT.p, d_workspace.p, d_knn.p);
  HIP_TRY(hipGetLastError());

  // inv as a CSR: count, scan, fill
  DevBuf<ull> d_count, d_inv_off, d_cursor, d_row_pairs, d_row_ranked, d_row_off;
  DevBuf<int32_t> d_inv;
  DevBuf<uint32_t> d_matrix;
  DevBuf<uint8_t> d_temp;
  if ((rc = d_count.alloc((size_t)N + 1)) || (rc = d_inv_off.alloc((size_t)N + 1)) || (rc = d_cursor.alloc((size_t)N + 1)) ||
      (rc = d_row_pairs.alloc((size_t)N + 1)) || (rc = d_row_ranked.alloc((size_t)N)) || (rc = d_row_off.alloc((size_t)N + 1)) ||
      (rc = d_inv.alloc(total)) || (rc = d_matrix.alloc((size_t)N * (size_t)W)))
    return rc;
  size_t temp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, d_count.p, d_inv_off.p, N + 1, nullptr));
  if ((rc = d_temp.alloc(temp_bytes))) return rc;
  HIP_TRY(hipMemset(d_count.p, 0, sizeof(ull) * ((size_t)N + 1)));
  HIP_TRY(hipMemset(d_row_pairs.p, 0, sizeof(ull) * ((size_t)N + 1)));
  const int grid_total = grid_of(total, kThreads);
  k_gm_count<<<grid_total, kThreads, 0, nullptr>>>((int64_t)total, d_knn.p, d_count.p);
  size_t want = temp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp.p, want, d_count.p, d_inv_off.p, N + 1, nullptr));
  HIP_TRY(hipMemcpyAsync(d_cursor.p, d_inv_off.p, sizeof(ull) * ((size_t)N + 1), hipMemcpyDeviceToDevice, nullptr));
  k_gm_fill<<<grid_total, kThreads, 0, nullptr>>>((int64_t)total, k, d_knn.p, d_cursor.p, d_inv.p);

  // the rows, their counts, the offsets (entry N of the scan is the total)
  k_gm_rows<<<N, kThreads, 2 * sizeof(uint32_t) * (size_t)W, nullptr>>>(N, k, W, d_knn.p, d_inv_off.p, d_inv.p, d_matrix.p,
                                                                        d_row_pairs.p, d_row_ranked.p);
  want = temp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp.p, want, d_row_pairs.p, d_row_off.p, N + 1, nullptr));
  HIP_TRY(hipGetLastError());
  ull count = 0;
  HIP_TRY(hipMemcpy(&count, d_row_off.p + N, sizeof(ull), hipMemcpyDeviceToHost));
  std::vector<ull> row_ranked((size_t)N);
  HIP_TRY(hipMemcpy(row_ranked.data(), d_row_ranked.p, sizeof(ull) * (size_t)N, hipMemcpyDeviceToHost));
  for (ull r : row_ranked) S.num_ranked_pairs += (int64_t)r;
  S.num_pairs = (int64_t)count;
  S.num_expanded_pairs = S.num_pairs - S.num_ranked_pairs;

  // everything that can fail runs before the first byte goes to the caller
  DevBuf<int32_t> d_pair1, d_pair2;
  const bool fits = S.num_pairs <= pair_capacity;
  if (fits) {
    if ((rc = d_pair1.alloc((size_t)count)) || (rc = d_pair2.alloc((size_t)count))) return rc;
    k_gm_emit<<<N, 64, 0, nullptr>>>(W, d_matrix.p, d_row_off.p, d_pair1.p, d_pair2.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  std::vector<uint64_t> keys;
  if (knn_index || knn_distance) {
    keys.resize(total);
    HIP_TRY(hipMemcpy(keys.data(), d_knn.p, sizeof(uint64_t) * total, hipMemcpyDeviceToHost));
  }
  if (fits && count) {
    HIP_TRY(hipMemcpy(pair_image1, d_pair1.p, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pair_image2, d_pair2.p, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost));
  }
  for (size_t t = 0; t < keys.size(); ++t) {
    if (knn_index) knn_index[t] = (int32_t)(uint32_t)keys[t];
    if (knn_distance) {
      const uint32_t bits = (uint32_t)(keys[t] >> 32);
      std::memcpy(knn_distance + t, &bits, sizeof(float));
    }
  }
  *num_pairs = S.num_pairs;
  if (stats) *stats = S;
  return 0;
}
