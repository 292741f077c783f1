// brute_force_matcher.hip -- BruteForceFeatureMatcher::MatchImagePair (matching/brute_force_feature_matcher.cc:48-115) for a
// whole match graph, the step of FeatureMatcher::MatchImages (matching/feature_matcher.cc:104-228) that makes the putative matches.
//
// A pair's squared-distance matrix is a GEMM: d(i, j) = |a_i|^2 + |b_j|^2 - 2 a_i . b_j, the expansion matching/distance.h:46-47
// names.  The dot products run on the exact FP32 MFMA (v_mfma_f32_32x32x2_f32), which is bit for bit an fmaf chain over ascending k
// with ONE accumulator per output element, so every distance is pinned:
//   dot = fmaf chain from +0.0f;  nrm = the same chain over d[k] * d[k];  t = nrm1 + nrm2;  d = max(fmaf(-2, dot, t), 0).
// distance(d2[j], d1[i]) of the reference's reverse pass is d(i, j) of the forward pass bit for bit, so ONE matrix serves both
// directions: row minima forward, column minima reverse.  The two nearest are taken under (distance, index) ascending; with d >= 0
// the key (float bits << 32 | index) makes that order a plain unsigned 64-bit minimum.
//
//   k_bf_norms   nrm of every feature of every image, once per call
//   k_bf_tiles   one workgroup per (pair, row block, column block) of a host-built work list: a 128 x 128 tile of the matrix, four
//                waves of 2 x 2 accumulators of 32 x 32 (instruction-level parallelism from independent tiles, never from a split K),
//                operands staged through LDS in K-chunks of 32 (the next chunk's global loads in flight under the MFMAs); the tile
//                then passes through LDS and one thread per row / column takes its top 2, written to a workspace as partials
//   k_bf_merge   per (pair, row) and (pair, column): the top 2 over the blocks' partials
//   k_bf_select  one workgroup per pair: ratio test in FP64, symmetric test, matches compacted in ascending feature1 order
// Pairs are processed in chunks sized to a fixed workspace budget; a pair's result does not depend on the chunk it falls into.
#include "device_util.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

namespace thip {
namespace {

constexpr int kTile = 128;                       // rows and columns of a workgroup's tile
constexpr int kChunkK = 32;                      // K-chunk staged through LDS
constexpr int kStageStride = kChunkK + 1;        // row stride of a staged operand: the 32 rows a half-wave reads fall into 32 banks
constexpr uint32_t kNoIndex = 0xffffffffu;
constexpr uint64_t kNoKey = 0x7f800000ffffffffull;   // (+inf, no index): what a side without candidates holds
constexpr size_t kWorkspaceBytes = (size_t)256 << 20;   // budget of the partial top-2s of one chunk of pairs
constexpr int kMaxPairsPerChunk = 32768;         // k_bf_merge takes the pair from blockIdx.y

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PairInfo {
  int64_t d1, d2;          // first feature of image 1 / image 2 among all features
  int32_t n1, n2;
  int32_t nrb, ncb;        // row blocks and column blocks of the pair
  int64_t rpart, cpart;    // first entry (two keys each) of the pair's row partials [ncb][n1] / column partials [nrb][n2]
  int64_t fwd, rev;        // first entry of the pair's merged rows / columns: the sum of n1 / n2 of the chunk's earlier pairs
};
struct Work { int32_t pair, rb, cb; };

__device__ __forceinline__ void push2(uint64_t key, uint64_t& k0, uint64_t& k1) {
  const bool lt0 = key < k0, lt1 = key < k1;   // selects, not branches: k0 / k1 stay in registers
  k1 = lt0 ? k0 : (lt1 ? key : k1);
  k0 = lt0 ? key : k0;
}

// *bad = 1 if a norm is not finite: a NaN or infinite descriptor value, or values whose squared norm overflows float
__global__ __launch_bounds__(256) void k_bf_norms(int64_t total, int dim, const float* __restrict__ desc, float* __restrict__ nrm,
                                                  int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float* d = desc + i * dim;
  float acc = 0.0f;
  for (int k = 0; k < dim; ++k) acc = __fmaf_rn(d[k], d[k], acc);
  nrm[i] = acc;
  if (!(fabsf(acc) <= FLT_MAX)) *bad = 1;
}

// One chunk of both operands, global -> registers: kVec (dim a multiple of 4) as 4 + 4 float4 per thread, otherwise 16 + 16
// floats.  Every load is unconditional at a clamped address (the block has at least one row and one column), the values beyond
// n1 / n2 / dim are then replaced by zeros (fma(0, 0, c) == c): loads that do not sit under a branch are issued together.
template <bool kVec>
struct Stage {
  static constexpr int kLoads = kVec ? 4 : 16;
  typedef typename std::conditional<kVec, float4, float>::type V;
  V a[kLoads], b[kLoads];
  // kVec: thread = (float4 tid & 7 of the chunk's 8, rows tid >> 3 + 32 i); else (k tid & 31, rows tid >> 5 + 8 i)
  __device__ __forceinline__ void load(const float* __restrict__ desc, const PairInfo& P, int row0, int col0, int dim, int kc, int tid) {
    const int k = kc + (kVec ? 4 * (tid & 7) : (tid & 31)), r0 = kVec ? tid >> 3 : tid >> 5;
    const bool kin = k < dim;
    const int kk = kin ? k : 0;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int r = r0 + (kTile / kLoads) * i;
      const float* pa = desc + (P.d1 + std::min(row0 + r, P.n1 - 1)) * dim + kk;
      const float* pb = desc + (P.d2 + std::min(col0 + r, P.n2 - 1)) * dim + kk;
      if constexpr (kVec) { a[i] = *reinterpret_cast<const float4*>(pa); b[i] = *reinterpret_cast<const float4*>(pb); }
      else { a[i] = *pa; b[i] = *pb; }
    }
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int r = r0 + (kTile / kLoads) * i;
      if (!(kin && row0 + r < P.n1)) a[i] = V{};
      if (!(kin && col0 + r < P.n2)) b[i] = V{};
    }
  }
  __device__ __forceinline__ void store(float* As, float* Bs, int tid) const {
    const int k = kVec ? 4 * (tid & 7) : (tid & 31), r0 = kVec ? tid >> 3 : tid >> 5;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      float* pa = As + (r0 + (kTile / kLoads) * i) * kStageStride + k;
      float* pb = Bs + (r0 + (kTile / kLoads) * i) * kStageStride + k;
      if constexpr (kVec) {
        pa[0] = a[i].x; pa[1] = a[i].y; pa[2] = a[i].z; pa[3] = a[i].w;
        pb[0] = b[i].x; pb[1] = b[i].y; pb[2] = b[i].z; pb[3] = b[i].w;
      } else { pa[0] = a[i]; pb[0] = b[i]; }
    }
  }
};

// the two smallest of a tile's row or column under (distance bits, position): the scan ascends, so a strict comparison keeps the
// earlier position of a tie.  Positions from `valid` on are padding (+inf): they leave as "no index".
struct Scan2 {
  uint32_t b0 = 0xffffffffu, b1 = 0xffffffffu;
  int i0 = kTile, i1 = kTile;
  __device__ __forceinline__ void push(uint32_t v, int i) {
    const bool lt0 = v < b0, lt1 = v < b1;
    b1 = lt0 ? b0 : (lt1 ? v : b1); i1 = lt0 ? i0 : (lt1 ? i : i1);
    b0 = lt0 ? v : b0; i0 = lt0 ? i : i0;
  }
  __device__ __forceinline__ void write(uint64_t* out, int first, int valid) const {
    valid = valid < kTile ? valid : kTile;   // i0 / i1 == kTile: nothing was pushed
    out[0] = ((uint64_t)b0 << 32) | (i0 < valid ? (uint32_t)(first + i0) : kNoIndex);
    out[1] = ((uint64_t)b1 << 32) | (i1 < valid ? (uint32_t)(first + i1) : kNoIndex);
  }
};

template <bool kVec>
__global__ __launch_bounds__(256) void k_bf_tiles(const Work* __restrict__ work, const PairInfo* __restrict__ pairs, int dim,
                                                  const float* __restrict__ desc, const float* __restrict__ nrm,
                                                  uint64_t* __restrict__ rowpart, uint64_t* __restrict__ colpart) {
  // the staged operands (2 x 128 x 33 floats) and, after the K loop, the 128 x 128 tile of distances share the block
  __shared__ float lds[kTile * kTile];
  const Work w = work[blockIdx.x];
  const PairInfo P = pairs[w.pair];
  const int row0 = w.rb * kTile, col0 = w.cb * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;   // the wave's 64 x 64 quarter of the tile
  float* As = lds;
  float* Bs = lds + kTile * kStageStride;
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[m][n][g] = 0.0f;

  Stage<kVec> st;
  st.load(desc, P, row0, col0, dim, 0, tid);
  for (int kc = 0; kc < dim; kc += kChunkK) {
    st.store(As, Bs, tid);
    __syncthreads();
    if (kc + kChunkK < dim) st.load(desc, P, row0, col0, dim, kc + kChunkK, tid);   // the next chunk, in flight under the MFMAs
    const float* ap = As + (wr + l31) * kStageStride + h;       // lane: A[row l & 31][k = l >> 5], B[k = l >> 5][column l & 31]
    const float* bp = Bs + (wc + l31) * kStageStride + h;
    auto step = [&](int s) {
      const float a0 = ap[2 * s], a1 = ap[32 * kStageStride + 2 * s];
      const float b0 = bp[2 * s], b1 = bp[32 * kStageStride + 2 * s];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    };
    // all 16 k pairs of the chunk, unrolled, so that the LDS reads run ahead of the MFMAs: beyond dim the staged operands are
    // zeros, and fma(0, 0, c) == c (c is never -0: the chain starts at +0), so a short last chunk costs time, not bits, and
    // one loop keeps the accumulators in one set of registers.
#pragma unroll
    for (int s = 0; s < kChunkK / 2; ++s) step(s);
    __syncthreads();
  }

  // the distances into LDS: element (r, c) at r * 128 + ((c + r) & 127), so that both the row scan (thread = row) and the column
  // scan (thread = column) walk distinct banks.  Rows beyond n1 and columns beyond n2 hold +inf.
  const float inf = __builtin_inff();
  float n2v[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) n2v[n] = nrm[P.d2 + std::min(col0 + wc + 32 * n + l31, P.n2 - 1)];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float n1v[16];
#pragma unroll
    for (int g = 0; g < 16; ++g)                            // C/D layout: column on the lane,
      n1v[g] = nrm[P.d1 + std::min(row0 + wr + 32 * m + (g & 3) + 8 * (g >> 2) + 4 * h, P.n1 - 1)];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int r = wr + 32 * m + (g & 3) + 8 * (g >> 2) + 4 * h;   // row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int c = wc + 32 * n + l31;
        const float t = n1v[g] + n2v[n];
        const float d = fmaxf(__fmaf_rn(-2.0f, acc[m][n][g], t), 0.0f);
        lds[r * kTile + ((c + r) & (kTile - 1))] = (row0 + r < P.n1 && col0 + c < P.n2) ? d : inf;
      }
    }
  }
  __syncthreads();
  Scan2 best;
  if (tid < kTile) {
    const int r = tid;
    if (row0 + r >= P.n1) return;
#pragma unroll 8
    for (int c = 0; c < kTile; ++c) best.push(__float_as_uint(lds[r * kTile + ((c + r) & (kTile - 1))]), c);
    best.write(rowpart + 2 * (P.rpart + (int64_t)w.cb * P.n1 + row0 + r), col0, P.n2 - col0);
  } else {
    const int c = tid - kTile;
    if (col0 + c >= P.n2) return;
#pragma unroll 8
    for (int r = 0; r < kTile; ++r) best.push(__float_as_uint(lds[r * kTile + ((c + r) & (kTile - 1))]), r);
    best.write(colpart + 2 * (P.cpart + (int64_t)w.rb * P.n2 + col0 + c), row0, P.n1 - row0);
  }
}

// blockIdx.y = pair; item i < n1: row i over the column blocks, n1 <= i < n1 + n2: column i - n1 over the row blocks
__global__ __launch_bounds__(256) void k_bf_merge(const PairInfo* __restrict__ pairs, const uint64_t* __restrict__ rowpart,
                                                  const uint64_t* __restrict__ colpart, uint64_t* __restrict__ fwd,
                                                  uint64_t* __restrict__ rev) {
  const PairInfo P = pairs[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P.n1 + P.n2) return;
  const bool row = i < P.n1;
  const int64_t e = row ? i : i - P.n1;
  const int nb = row ? P.ncb : P.nrb;
  const int64_t n = row ? P.n1 : P.n2;   // block b's partials of all rows (columns) lie together: neighbouring threads, neighbouring keys
  const uint64_t* in = row ? rowpart + 2 * (P.rpart + e) : colpart + 2 * (P.cpart + e);
  uint64_t k0 = kNoKey, k1 = kNoKey;
  for (int b = 0; b < nb; ++b) { push2(in[2 * b * n], k0, k1); push2(in[2 * b * n + 1], k0, k1); }
  uint64_t* out = row ? fwd + 2 * (P.fwd + e) : rev + 2 * (P.rev + e);
  out[0] = k0; out[1] = k1;
}

__device__ __forceinline__ bool passes_ratio(uint64_t k0, uint64_t k1, int use_ratio, double sq) {
  if ((uint32_t)k0 == kNoIndex) return false;   // a side without candidates yields nothing
  return !use_ratio || (double)__uint_as_float((uint32_t)(k0 >> 32)) < sq * (double)__uint_as_float((uint32_t)(k1 >> 32));
}

// One workgroup per pair: the forward matches that pass the ratio test (and, if symmetric, whose feature2 passed the reverse test
// with this feature1 as its nearest: IntersectMatches, feature_matcher_utils.cc:48-70) in ascending feature1 order, written from
// the pair's slot P.fwd on; counts[pair] = their number.
__global__ __launch_bounds__(256) void k_bf_select(const PairInfo* __restrict__ pairs, const uint64_t* __restrict__ fwd,
                                                   const uint64_t* __restrict__ rev, int symmetric, int use_ratio, double sq,
                                                   int32_t* __restrict__ m_f1, int32_t* __restrict__ m_f2, float* __restrict__ m_d,
                                                   int32_t* __restrict__ counts) {
  __shared__ int wsum[4];
  const PairInfo P = pairs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int i0 = 0; i0 < P.n1; i0 += 256) {
    const int i = i0 + tid;
    bool keep = false;
    uint64_t k0 = kNoKey;
    if (i < P.n1) {
      k0 = fwd[2 * (P.fwd + i)];
      keep = passes_ratio(k0, fwd[2 * (P.fwd + i) + 1], use_ratio, sq);
      if (keep && symmetric) {
        const uint64_t* r = rev + 2 * (P.rev + (uint32_t)k0);
        keep = passes_ratio(r[0], r[1], use_ratio, sq) && (uint32_t)r[0] == (uint32_t)i;
      }
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { if (q < wave) off += wsum[q]; total += wsum[q]; }
    if (keep) {
      const int64_t at = P.fwd + off + __popcll(bal & (((uint64_t)1 << lane) - 1));
      m_f1[at] = i; m_f2[at] = (int32_t)(uint32_t)k0; m_d[at] = __uint_as_float((uint32_t)(k0 >> 32));
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = base;
}

// The device side of one call: every image's descriptors and norms, and the workspace of the largest chunk.
struct Matcher {
  int dim = 0;
  DevBuf<float> desc, nrm;
  DevBuf<uint64_t> rowpart, colpart, fwd, rev;
  DevBuf<PairInfo> pairs;
  DevBuf<Work> work;
  std::vector<PairInfo> hp;
  std::vector<Work> hw;
  int64_t sum1 = 0, sum2 = 0;   // features of image 1 / image 2 summed over the chunk

  int norms(int64_t total) {
    int rc = nrm.alloc((size_t)total);
    if (rc || !total) return rc;
    DevBuf<int> bad;
    if ((rc = bad.alloc(1))) return rc;
    HIP_TRY(hipMemset(bad.p, 0, sizeof(int)));
    k_bf_norms<<<grid_of((size_t)total, 256), 256, 0, nullptr>>>(total, dim, desc.p, nrm.p, bad.p);
    HIP_TRY(hipGetLastError());
    int h_bad = 0;
    HIP_TRY(hipMemcpy(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost));
    // with such a value every distance to the feature is NaN, and the clamp at 0 would make it the nearest of every query
    if (h_bad) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a descriptor is not finite (or its squared norm overflows float)");
    return 0;
  }
  static size_t partial_bytes(int64_t n1, int64_t n2) {
    const int64_t nrb = (n1 + kTile - 1) / kTile, ncb = (n2 + kTile - 1) / kTile;
    return (size_t)(n1 * ncb + n2 * nrb) * 2 * sizeof(uint64_t);
  }
  // lays out one chunk: pair k has the features [o1[k], o1[k] + n1[k]) and [o2[k], o2[k] + n2[k])
  void plan(int count, const int64_t* o1, const int32_t* n1, const int64_t* o2, const int32_t* n2) {
    hp.resize((size_t)count); hw.clear();
    int64_t rp = 0, cp = 0;
    sum1 = sum2 = 0;
    for (int k = 0; k < count; ++k) {
      PairInfo& P = hp[(size_t)k];
      P.d1 = o1[k]; P.d2 = o2[k]; P.n1 = n1[k]; P.n2 = n2[k];
      P.nrb = (n1[k] + kTile - 1) / kTile; P.ncb = (n2[k] + kTile - 1) / kTile;
      P.rpart = rp; P.cpart = cp; P.fwd = sum1; P.rev = sum2;
      rp += (int64_t)P.n1 * P.ncb; cp += (int64_t)P.n2 * P.nrb; sum1 += P.n1; sum2 += P.n2;
      for (int rb = 0; rb < P.nrb; ++rb) for (int cb = 0; cb < P.ncb; ++cb) hw.push_back(Work{k, rb, cb});
    }
  }
  // the planned chunk's merged top 2 per row (fwd) and per column (rev); the buffers must hold the chunk
  int knn() {
    const int count = (int)hp.size();
    HIP_TRY(hipMemcpy(pairs.p, hp.data(), sizeof(PairInfo) * hp.size(), hipMemcpyHostToDevice));
    if (!hw.empty()) {
      HIP_TRY(hipMemcpy(work.p, hw.data(), sizeof(Work) * hw.size(), hipMemcpyHostToDevice));
      if (dim % 4 == 0) k_bf_tiles<true><<<(unsigned)hw.size(), 256, 0, nullptr>>>(work.p, pairs.p, dim, desc.p, nrm.p, rowpart.p, colpart.p);
      else k_bf_tiles<false><<<(unsigned)hw.size(), 256, 0, nullptr>>>(work.p, pairs.p, dim, desc.p, nrm.p, rowpart.p, colpart.p);
      HIP_TRY(hipGetLastError());
    }
    int64_t most = 0;
    for (const PairInfo& P : hp) most = std::max(most, (int64_t)P.n1 + P.n2);
    if (most) {
      k_bf_merge<<<dim3((unsigned)grid_of((size_t)most, 256), (unsigned)count), 256, 0, nullptr>>>(pairs.p, rowpart.p, colpart.p, fwd.p, rev.p);
      HIP_TRY(hipGetLastError());
    }
    return 0;
  }
};

void decode(const std::vector<uint64_t>& keys, int64_t n, float* dist, int32_t* index) {
  for (int64_t i = 0; i < 2 * n; ++i) {
    const uint32_t bits = (uint32_t)(keys[(size_t)i] >> 32), idx = (uint32_t)keys[(size_t)i];
    std::memcpy(&dist[i], &bits, sizeof(float));
    index[i] = idx == kNoIndex ? -1 : (int32_t)idx;
  }
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" void theia_hip_brute_force_options_default(theia_brute_force_options* o) {
  if (!o) return;
  o->keep_only_symmetric_matches = 1;   // feature_matcher_options.h:66-87
  o->use_lowes_ratio = 1;
  o->lowes_ratio = 0.8f;
  o->min_num_feature_matches = 30;
  o->max_pairs_per_launch = 0;
}

extern "C" int theia_hip_brute_force_knn2(int32_t n1, int32_t n2, int32_t dim, const float* desc1, const float* desc2, float* fwd_dist,
                                          int32_t* fwd_index, float* rev_dist, int32_t* rev_index) {
  if (n1 < 0 || n2 < 0 || dim < 1) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad sizes");
  if ((n1 && (!desc1 || !fwd_dist || !fwd_index)) || (n2 && (!desc2 || !rev_dist || !rev_index)))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (n1 + (int64_t)n2 == 0) return 0;
  int rc = ensure_device();
  if (rc) return rc;
  Matcher M;
  M.dim = dim;
  const size_t e1 = (size_t)n1 * dim, e2 = (size_t)n2 * dim;
  if ((rc = M.desc.alloc(e1 + e2))) return rc;
  if (e1) HIP_TRY(hipMemcpy(M.desc.p, desc1, e1 * sizeof(float), hipMemcpyHostToDevice));
  if (e2) HIP_TRY(hipMemcpy(M.desc.p + e1, desc2, e2 * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = M.norms((int64_t)n1 + n2))) return rc;
  const int64_t o1 = 0, o2 = n1;
  M.plan(1, &o1, &n1, &o2, &n2);
  if ((rc = M.rowpart.alloc((size_t)n1 * M.hp[0].ncb * 2)) || (rc = M.colpart.alloc((size_t)n2 * M.hp[0].nrb * 2)) ||
      (rc = M.fwd.alloc((size_t)n1 * 2)) || (rc = M.rev.alloc((size_t)n2 * 2)) || (rc = M.pairs.alloc(1)) || (rc = M.work.alloc(M.hw.size())))
    return rc;
  if ((rc = M.knn())) return rc;
  std::vector<uint64_t> kf((size_t)n1 * 2), kr((size_t)n2 * 2);
  if (n1) HIP_TRY(hipMemcpy(kf.data(), M.fwd.p, kf.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (n2) HIP_TRY(hipMemcpy(kr.data(), M.rev.p, kr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  decode(kf, n1, fwd_dist, fwd_index);
  decode(kr, n2, rev_dist, rev_index);
  return 0;
}

extern "C" int theia_hip_brute_force_match_pairs(int32_t num_images, const int64_t* feat_off, int32_t dim, const float* descriptors,
                                                 int32_t num_pairs, const int32_t* pair_image1, const int32_t* pair_image2,
                                                 const theia_brute_force_options* options, uint8_t* pair_ok, int64_t* match_off,
                                                 int32_t* match_feature1, int32_t* match_feature2, float* match_distance) {
  if (num_images < 0 || dim < 1 || num_pairs < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad sizes");
  if (!options || options->max_pairs_per_launch < 0 || !(options->lowes_ratio >= 0.0f))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad options");
  if (!feat_off || !match_off) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (feat_off[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must start at 0");
  for (int i = 0; i < num_images; ++i) {
    if (feat_off[i + 1] < feat_off[i]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing");
    if (feat_off[i + 1] - feat_off[i] >= ((int64_t)1 << 30)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "too many features in an image");
  }
  const int64_t total = feat_off[num_images];
  if (num_pairs && (!pair_image1 || !pair_image2 || !pair_ok)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (total && !descriptors) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  int64_t capacity = 0;
  for (int k = 0; k < num_pairs; ++k) {
    if (pair_image1[k] < 0 || pair_image1[k] >= num_images || pair_image2[k] < 0 || pair_image2[k] >= num_images)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "image index out of range");
    capacity += feat_off[pair_image1[k] + 1] - feat_off[pair_image1[k]];
  }
  if (capacity && (!match_feature1 || !match_feature2 || !match_distance)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  if (num_pairs == 0) { match_off[0] = 0; return 0; }
  int rc = ensure_device();
  if (rc) return rc;

  // chunks of consecutive pairs: as many as the workspace budget holds (always one), at most max_pairs_per_launch if set
  std::vector<int64_t> o1((size_t)num_pairs), o2((size_t)num_pairs);
  std::vector<int32_t> n1((size_t)num_pairs), n2((size_t)num_pairs);
  for (int k = 0; k < num_pairs; ++k) {
    o1[k] = feat_off[pair_image1[k]]; n1[k] = (int32_t)(feat_off[pair_image1[k] + 1] - o1[k]);
    o2[k] = feat_off[pair_image2[k]]; n2[k] = (int32_t)(feat_off[pair_image2[k] + 1] - o2[k]);
  }
  const int cap = options->max_pairs_per_launch ? std::min(options->max_pairs_per_launch, kMaxPairsPerChunk) : kMaxPairsPerChunk;
  std::vector<int> chunk_begin{0};
  size_t most_rp = 0, most_cp = 0, most_s1 = 0, most_s2 = 0, most_work = 0, most_pairs = 0;
  {
    size_t bytes = 0, rp = 0, cp = 0, s1 = 0, s2 = 0, wk = 0;
    auto close = [&](int k) {
      most_rp = std::max(most_rp, rp); most_cp = std::max(most_cp, cp); most_s1 = std::max(most_s1, s1); most_s2 = std::max(most_s2, s2);
      most_work = std::max(most_work, wk); most_pairs = std::max(most_pairs, (size_t)(k - chunk_begin.back()));
    };
    for (int k = 0; k < num_pairs; ++k) {
      const size_t b = Matcher::partial_bytes(n1[k], n2[k]);
      if (k > chunk_begin.back() && (bytes + b > kWorkspaceBytes || k - chunk_begin.back() >= cap)) {
        close(k);
        chunk_begin.push_back(k);
        bytes = rp = cp = s1 = s2 = wk = 0;
      }
      const size_t nrb = (size_t)(n1[k] + kTile - 1) / kTile, ncb = (size_t)(n2[k] + kTile - 1) / kTile;
      bytes += b; rp += (size_t)n1[k] * ncb; cp += (size_t)n2[k] * nrb; s1 += n1[k]; s2 += n2[k]; wk += nrb * ncb;
    }
    close(num_pairs);
    chunk_begin.push_back(num_pairs);
  }
  if (most_work >= ((size_t)1 << 31)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a pair is too large for one launch");

  Matcher M;
  M.dim = dim;
  DevBuf<int32_t> d_f1, d_f2, d_cnt;
  DevBuf<float> d_md;
  if ((rc = M.desc.up(descriptors, (size_t)total * dim)) || (rc = M.norms(total)) || (rc = M.rowpart.alloc(most_rp * 2)) ||
      (rc = M.colpart.alloc(most_cp * 2)) || (rc = M.fwd.alloc(most_s1 * 2)) || (rc = M.rev.alloc(most_s2 * 2)) ||
      (rc = M.pairs.alloc(most_pairs)) || (rc = M.work.alloc(most_work)) || (rc = d_f1.alloc(most_s1)) || (rc = d_f2.alloc(most_s1)) ||
      (rc = d_md.alloc(most_s1)) || (rc = d_cnt.alloc(most_pairs)))
    return rc;
  match_off[0] = 0;
  const float lr = options->lowes_ratio * options->lowes_ratio;   // the reference squares the float option, then widens
  const double sq = (double)lr;
  std::vector<int32_t> h_f1(most_s1), h_f2(most_s1), h_cnt(most_pairs);
  std::vector<float> h_md(most_s1);
  int64_t at = 0;
  for (size_t c = 0; c + 1 < chunk_begin.size(); ++c) {
    const int k0 = chunk_begin[c], count = chunk_begin[c + 1] - k0;
    M.plan(count, &o1[k0], &n1[k0], &o2[k0], &n2[k0]);
    if ((rc = M.knn())) return rc;
    k_bf_select<<<(unsigned)count, 256, 0, nullptr>>>(M.pairs.p, M.fwd.p, M.rev.p, options->keep_only_symmetric_matches != 0,
                                                      options->use_lowes_ratio != 0, sq, d_f1.p, d_f2.p, d_md.p, d_cnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h_cnt.data(), d_cnt.p, sizeof(int32_t) * count, hipMemcpyDeviceToHost));
    if (M.sum1) {
      HIP_TRY(hipMemcpy(h_f1.data(), d_f1.p, sizeof(int32_t) * M.sum1, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(h_f2.data(), d_f2.p, sizeof(int32_t) * M.sum1, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(h_md.data(), d_md.p, sizeof(float) * M.sum1, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < count; ++k) {
      const PairInfo& P = M.hp[(size_t)k];
      const int32_t m = h_cnt[(size_t)k];
      const bool ok = m >= options->min_num_feature_matches;   // :114; the early return of :82-84 is implied by it
      pair_ok[k0 + k] = ok ? 1 : 0;
      if (ok && m) {
        std::memcpy(match_feature1 + at, h_f1.data() + P.fwd, sizeof(int32_t) * m);
        std::memcpy(match_feature2 + at, h_f2.data() + P.fwd, sizeof(int32_t) * m);
        std::memcpy(match_distance + at, h_md.data() + P.fwd, sizeof(float) * m);
        at += m;
      }
      match_off[k0 + k + 1] = at;
    }
  }
  return 0;
}
