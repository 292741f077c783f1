// track_builder.hip -- TrackBuilder::BuildTracks (sfm/track_builder.cc:62-77, :156-209 over math/graph/connected_components.h:
// 87-119, then Reconstruction::AddTrack, reconstruction.cc:314-351) for the indexed matches of a whole match graph: the link
// between the matcher / the indexed verification and everything that consumes tracks.  The rule, the stated orders and the stated
// deviations are in include/theia_hip.h and DESIGN.md 3.6n.
//
// The fact the design rests on: every edge lies inside one component of the UNCAPPED graph, and the reference's capped union sees,
// on the nodes of such a component, only that component's edges in their relative order.  So the reference's partition is: the
// uncapped components of at most max_track_length nodes as they are, every larger one replaced by the sequential capped rule over
// its own edges in input order.  The first part is connected components, done here on the device; the second is sequential by
// definition and runs on the host over the compacted edges of the oversized components only.
//
//   k_tb_edges     one lane per edge: its pair by bisection of match_off, the feature indices checked against their views, the
//                  edge as (node1 << 32 | node2) with node = feat_off[view] + feature, the two nodes marked present
//   k_tb_hook      lock-free union-find hooking, one lane per edge (below)
//   k_tb_flatten   parent[v] = root(v): the label of a component is its smallest node id
//   k_tb_sizes     size[label] by integer atomic adds;  k_tb_census  the counts of nodes, components and oversized components
//   k_tb_flag_nodes + DeviceSelect::Flagged + DeviceScan::ExclusiveSum   the oversized components' nodes, numbered in ascending id
//   k_tb_flag_edges + DeviceSelect::Flagged + k_tb_rank_edges   their edges, input order kept, between those numbers: what the
//                  host replay reads, so that it is a plain array union-find
//   k_tb_relabel   the replayed nodes' new labels (again the smallest node id of each part), then k_tb_sizes once more
//   DeviceSelect::Flagged over the node ids, k_tb_labels, DeviceRadixSort::SortPairs (stable) by label: nodes by (label, node id)
//   k_tb_classify  per sorted node: its view, component head, min_track_length on the node count, inconsistent iff the predecessor
//                  in the segment has the same view;  DeviceScan::ExclusiveSum over (track head << 32 | observation kept)
//   k_tb_emit      track_off / obs_view / obs_feature / obs_track
//
// The hooking.  parent[v] = v at the start, and every write keeps the invariant  parent[v] <= v :
//   - find() follows parent and halves the path by storing a grandparent, an ancestor, which is <= the parent <= v;
//   - an edge hooks the LARGER of its two roots under the smaller with compare-and-swap(parent[hi], hi, lo), lo < hi.
// A strictly decreasing walk ends, so find() takes at most v steps and no cycle can form; a root is the smallest node of its tree.
// A compare-and-swap that fails returns a value < hi (hi was hooked by another lane meanwhile); the lane continues from that value,
// so (larger root + smaller root) strictly decreases per retry: every loop is bounded by the node ids alone.  No lane waits for
// another lane's progress: there is no flag to spin on and no lock.  A stale read of parent[] yields an older ancestor, which is
// still an ancestor; only the compare-and-swap decides a hook.  Whatever the interleaving, every component ends as one tree whose
// root is its smallest node id, so the labels, and with them every output, are the same on every run.  Everything is integer.
#include "device_util.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

namespace thip {
namespace {

constexpr int kThreads = 256;
enum { kNodes = 0, kComponents, kOversized, kSmall, kInconsistent, kBad, kNumCounters };

thread_local theia_track_builder_timings g_timings{};

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one atomic per wave: the number of its lanes with pred.  Called by every lane that is still in the kernel.
__device__ __forceinline__ void count_if(bool pred, unsigned long long* counter) {
  const unsigned long long m = __ballot(pred);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// first k of [0, n) with off[k + 1] > x; the caller guarantees off[0] <= x < off[n]
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid + 1] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_tb_edges(int64_t M, int num_pairs, const int64_t* __restrict__ match_off,
                                                       const int32_t* __restrict__ pv1, const int32_t* __restrict__ pv2,
                                                       const int64_t* __restrict__ feat_off, const int32_t* __restrict__ f1,
                                                       const int32_t* __restrict__ f2, uint64_t* __restrict__ edge,
                                                       uint8_t* __restrict__ present, unsigned long long* __restrict__ counters) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= M) return;
  const int k = segment_of(match_off, num_pairs, e);
  const int v1 = pv1[k], v2 = pv2[k];   // checked on the host: inside [0, num_views), different
  const int64_t a = f1[e], b = f2[e];
  const bool bad = a < 0 || b < 0 || a >= feat_off[v1 + 1] - feat_off[v1] || b >= feat_off[v2 + 1] - feat_off[v2];
  count_if(bad, counters + kBad);
  if (bad) { edge[e] = 0; return; }
  const uint32_t n1 = (uint32_t)(feat_off[v1] + a), n2 = (uint32_t)(feat_off[v2] + b);   // < feat_off[num_views] < 2^31
  edge[e] = (uint64_t)n1 << 32 | n2;
  present[n1] = 1;
  present[n2] = 1;
}

__global__ __launch_bounds__(kThreads) void k_tb_init(int N, int* __restrict__ parent) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < N) parent[v] = v;
}

// the root of v's tree at some moment of the call, with path halving; at most v steps (parent[] strictly decreases along the walk)
__device__ __forceinline__ int find_halving(int* parent, int v) {
  for (;;) {
    const int p = ld(parent + v);
    if (p == v) return v;
    const int g = ld(parent + p);
    if (g == p) return p;
    st(parent + v, g);   // g < p < v: an ancestor of v, and v is no root, so no compare-and-swap expects parent[v] == v
    v = g;
  }
}

__global__ __launch_bounds__(kThreads) void k_tb_hook(int64_t M, const uint64_t* __restrict__ edge, int* parent) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= M) return;
  int a = find_halving(parent, (int)(edge[e] >> 32)), b = find_halving(parent, (int)(uint32_t)edge[e]);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) break;                  // hooked: hi was a root and now hangs under lo < hi
    a = find_halving(parent, seen);         // seen < hi: another lane hooked hi first; go on from where it hangs
    b = find_halving(parent, lo);           // <= lo
  }
}

__global__ __launch_bounds__(kThreads) void k_tb_flatten(int N, const uint8_t* __restrict__ present, int* parent) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= N || !present[v]) return;
  int r = v;
  for (int p = ld(parent + r); p != r; p = ld(parent + r)) r = p;   // reads only; other lanes' stores are roots of the same tree
  st(parent + v, r);
}

__global__ __launch_bounds__(kThreads) void k_tb_sizes(int N, const uint8_t* __restrict__ present, const int* __restrict__ label,
                                                       int* __restrict__ size) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < N && present[v]) atomicAdd(size + label[v], 1);
}

__global__ __launch_bounds__(kThreads) void k_tb_census(int N, const uint8_t* __restrict__ present, const int* __restrict__ label,
                                                        const int* __restrict__ size, int max_len,
                                                        unsigned long long* __restrict__ counters) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= N) return;
  const bool here = present[v] != 0, head = here && label[v] == v;
  count_if(here, counters + kNodes);
  count_if(head, counters + kComponents);
  count_if(head && size[v] > max_len, counters + kOversized);
}

__global__ __launch_bounds__(kThreads) void k_tb_flag_edges(int64_t M, const uint64_t* __restrict__ edge, const int* __restrict__ label,
                                                            const int* __restrict__ size, int max_len, uint8_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e < M) flag[e] = size[label[(int)(edge[e] >> 32)]] > max_len;   // both ends lie in one component
}

// flag[v] = 1 for the nodes of the oversized components; its exclusive sum numbers them 0 .. R - 1 in ascending node id
__global__ __launch_bounds__(kThreads) void k_tb_flag_nodes(int N, const uint8_t* __restrict__ present, const int* __restrict__ label,
                                                            const int* __restrict__ size, int max_len, int* __restrict__ flag) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < N) flag[v] = present[v] && size[label[v]] > max_len;
}

// the replay's edges from node ids to those numbers
__global__ __launch_bounds__(kThreads) void k_tb_rank_edges(int count, const int* __restrict__ rank, uint64_t* __restrict__ edge) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < count) edge[i] = (uint64_t)(uint32_t)rank[(int)(edge[i] >> 32)] << 32 | (uint32_t)rank[(int)(uint32_t)edge[i]];
}

// node[i]: the i-th replayed node; root[i]: the number of its part's smallest node
__global__ __launch_bounds__(kThreads) void k_tb_relabel(int R, const int* __restrict__ node, const int* __restrict__ root,
                                                         int* __restrict__ label) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < R) label[node[i]] = node[root[i]];
}

__global__ __launch_bounds__(kThreads) void k_tb_labels(int n, const int* __restrict__ node, const int* __restrict__ label,
                                                        int* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = label[node[i]];
}

// sl / sn: the nodes' labels and ids in (label, node id) order.  flags[i] = (i opens a track) << 32 | (i is an observation)
__global__ __launch_bounds__(kThreads) void k_tb_classify(int n, const int* __restrict__ sl, const int* __restrict__ sn,
                                                          const int* __restrict__ size, const int64_t* __restrict__ feat_off,
                                                          int num_views, int min_len, int* __restrict__ view,
                                                          uint64_t* __restrict__ flags, unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int v = segment_of(feat_off, num_views, sn[i]);
  view[i] = v;
  const bool head = i == 0 || sl[i - 1] != sl[i];
  const bool kept = size[sl[i]] >= min_len;
  // within a segment the node ids ascend, so a view's features are adjacent and its first is the lowest feature index
  const bool inconsistent = kept && !head && segment_of(feat_off, num_views, sn[i - 1]) == v;
  count_if(head && !kept, counters + kSmall);
  count_if(inconsistent, counters + kInconsistent);
  flags[i] = (uint64_t)(head && kept) << 32 | (uint64_t)(kept && !inconsistent);
}

__global__ __launch_bounds__(kThreads) void k_tb_emit(int n, const int* __restrict__ sn, const int* __restrict__ view,
                                                      const uint64_t* __restrict__ flags, const uint64_t* __restrict__ before,
                                                      const int64_t* __restrict__ feat_off, int64_t* __restrict__ track_off,
                                                      int32_t* __restrict__ obs_view, int32_t* __restrict__ obs_feature,
                                                      int32_t* __restrict__ obs_track) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n || !(uint32_t)flags[i]) return;
  const uint32_t at = (uint32_t)before[i];                              // observations before i: < n
  const uint32_t track = (uint32_t)((before[i] + flags[i]) >> 32) - 1;   // tracks opened up to and including i, minus one
  obs_view[at] = view[i];
  obs_feature[at] = (int32_t)(sn[i] - feat_off[view[i]]);
  obs_track[at] = (int32_t)track;
  if (flags[i] >> 32) track_off[track] = at;
}

// the reference's capped union over the edges of the oversized components, in input order, on a plain array union-find over the
// replayed nodes' numbers (ascending with the node ids).  The decision reads only the sizes, so hooking the larger root under the
// smaller changes nothing and leaves each part's smallest node as its root.  root[i]: the number of the smallest node of i's part.
void replay_capped(const std::vector<uint64_t>& edges, int num_nodes, int64_t max_len, std::vector<int>& root) {
  const size_t n = (size_t)num_nodes;
  root.resize(n);
  std::vector<int>& parent = root;
  std::vector<int64_t> size(n, 1);
  for (size_t i = 0; i < n; ++i) parent[i] = (int)i;
  auto find = [&](int v) {
    while (parent[(size_t)v] != v) { parent[(size_t)v] = parent[(size_t)parent[(size_t)v]]; v = parent[(size_t)v]; }
    return v;
  };
  for (uint64_t e : edges) {
    int a = find((int)(e >> 32)), b = find((int)(uint32_t)e);
    if (a == b || size[(size_t)a] + size[(size_t)b] > max_len) continue;
    if (a > b) std::swap(a, b);
    parent[(size_t)b] = a;
    size[(size_t)a] += size[(size_t)b];
  }
  for (size_t i = 0; i < n; ++i) root[i] = find((int)i);   // root is parent: a node's entry becomes its root, a root's stays
}

}  // namespace
}  // namespace thip

using namespace thip;

extern "C" void theia_hip_track_builder_options_default(theia_track_builder_options* o) {
  if (!o) return;
  o->min_track_length = 2;    // reconstruction_builder.h:81-85
  o->max_track_length = 50;
}

extern "C" int theia_hip_track_builder_last_timings(theia_track_builder_timings* out) {
  if (!out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out = g_timings;
  return 0;
}

extern "C" int theia_hip_build_tracks(int32_t num_views, const int64_t* feat_off, int32_t num_pairs, const int32_t* pair_view1,
                                      const int32_t* pair_view2, const int64_t* match_off, const int32_t* feature1,
                                      const int32_t* feature2, const theia_track_builder_options* options, int64_t* track_off,
                                      int32_t* obs_view, int32_t* obs_feature, int32_t* obs_track, theia_track_builder_stats* stats) {
  if (num_views < 0 || num_pairs < 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "bad sizes");
  if (!options || !feat_off || !match_off || !track_off) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (options->min_track_length < 2)   // a singleton would reach AddTrack's CHECK (reconstruction.cc:314-351)
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "min_track_length must be at least 2");
  if (options->max_track_length <= 0)  // connected_components.h:77
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "max_track_length must be positive");
  if (feat_off[0] != 0 || match_off[0] != 0) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "offsets must start at 0");
  for (int i = 0; i < num_views; ++i)
    if (feat_off[i + 1] < feat_off[i]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "feat_off must be non-decreasing");
  if (num_pairs && (!pair_view1 || !pair_view2)) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  for (int k = 0; k < num_pairs; ++k) {
    if (match_off[k + 1] < match_off[k]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "match_off must be non-decreasing");
    if (pair_view1[k] < 0 || pair_view1[k] >= num_views || pair_view2[k] < 0 || pair_view2[k] >= num_views)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view index out of range");
    if (pair_view1[k] == pair_view2[k] && match_off[k + 1] > match_off[k])   // track_builder.cc:66
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "a correspondence inside one view");
  }
  const int64_t total = feat_off[num_views], M = match_off[num_pairs];
  if (total >= ((int64_t)1 << 31) || M >= ((int64_t)1 << 31))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "2^31 or more features or correspondences");
  if (M && (!feature1 || !feature2 || !obs_view || !obs_feature || !obs_track))
    return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null array");
  theia_track_builder_stats S{};
  if (M == 0) {
    track_off[0] = 0;
    if (stats) *stats = S;
    return 0;
  }
  int rc = ensure_device();
  if (rc) return rc;
  const int N = (int)total, max_len = options->max_track_length, min_len = options->min_track_length;
  theia_track_builder_timings T{};
  const auto t_start = std::chrono::steady_clock::now();

  // upload; validation and node marking
  DevBuf<int64_t> d_feat_off, d_match_off;
  DevBuf<int32_t> d_pv1, d_pv2, d_f1, d_f2;
  DevBuf<uint64_t> d_edge;
  DevBuf<uint8_t> d_present, d_eflag;
  DevBuf<unsigned long long> d_counters;
  DevBuf<int> d_parent, d_size, d_count;
  if ((rc = d_feat_off.up(feat_off, (size_t)num_views + 1)) || (rc = d_match_off.up(match_off, (size_t)num_pairs + 1)) ||
      (rc = d_pv1.up(pair_view1, (size_t)num_pairs)) || (rc = d_pv2.up(pair_view2, (size_t)num_pairs)) ||
      (rc = d_f1.up(feature1, (size_t)M)) || (rc = d_f2.up(feature2, (size_t)M)) || (rc = d_edge.alloc((size_t)M)) ||
      (rc = d_present.alloc((size_t)N)) || (rc = d_eflag.alloc((size_t)M)) || (rc = d_counters.alloc(kNumCounters)) ||
      (rc = d_parent.alloc((size_t)N)) || (rc = d_size.alloc((size_t)N)) || (rc = d_count.alloc(1)))
    return rc;
  HIP_TRY(hipMemset(d_present.p, 0, (size_t)N));
  HIP_TRY(hipMemset(d_size.p, 0, sizeof(int) * (size_t)N));
  HIP_TRY(hipMemset(d_counters.p, 0, sizeof(unsigned long long) * kNumCounters));
  const int grid_m = grid_of((size_t)M, kThreads), grid_n = grid_of((size_t)N, kThreads);
  k_tb_edges<<<grid_m, kThreads, 0, nullptr>>>(M, num_pairs, d_match_off.p, d_pv1.p, d_pv2.p, d_feat_off.p, d_f1.p, d_f2.p, d_edge.p,
                                               d_present.p, d_counters.p);
  HIP_TRY(hipGetLastError());
  unsigned long long counters[kNumCounters];
  HIP_TRY(hipMemcpy(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost));
  if (counters[kBad]) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "%llu feature indices lie outside their views", counters[kBad]);
  T.upload_ms = ms_since(t_start);

  // the components without the cap, their sizes, the edges of the oversized ones
  const auto t_components = std::chrono::steady_clock::now();
  k_tb_init<<<grid_n, kThreads, 0, nullptr>>>(N, d_parent.p);
  k_tb_hook<<<grid_m, kThreads, 0, nullptr>>>(M, d_edge.p, d_parent.p);
  k_tb_flatten<<<grid_n, kThreads, 0, nullptr>>>(N, d_present.p, d_parent.p);
  k_tb_sizes<<<grid_n, kThreads, 0, nullptr>>>(N, d_present.p, d_parent.p, d_size.p);
  k_tb_census<<<grid_n, kThreads, 0, nullptr>>>(N, d_present.p, d_parent.p, d_size.p, max_len, d_counters.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost));
  S.num_nodes = (int64_t)counters[kNodes];
  S.num_components = (int64_t)counters[kComponents];
  S.num_oversized_components = (int64_t)counters[kOversized];
  const int n = (int)S.num_nodes;   // >= 2: M > 0 and every edge joins two views

  // one workspace for the library calls: the largest any of them asks for
  DevBuf<int> d_nodes, d_labels, d_sn, d_sl, d_view;
  DevBuf<uint64_t> d_flags, d_before, d_sel;
  DevBuf<uint8_t> d_temp;
  if ((rc = d_nodes.alloc((size_t)n)) || (rc = d_labels.alloc((size_t)n)) || (rc = d_sn.alloc((size_t)n)) ||
      (rc = d_sl.alloc((size_t)n)) || (rc = d_view.alloc((size_t)n)) || (rc = d_flags.alloc((size_t)n)) ||
      (rc = d_before.alloc((size_t)n)))
    return rc;
  int label_bits = 1;
  while (label_bits < 31 && ((int64_t)1 << label_bits) < N) ++label_bits;   // a label is a node id < N
  hipcub::CountingInputIterator<int> ids(0);
  size_t temp_bytes = 0, want = 0;
  HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, want, ids, d_present.p, d_nodes.p, d_count.p, N, nullptr));
  temp_bytes = std::max(temp_bytes, want);
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, want, d_labels.p, d_sl.p, d_nodes.p, d_sn.p, n, 0, label_bits, nullptr));
  temp_bytes = std::max(temp_bytes, want);
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, want, d_flags.p, d_before.p, n, nullptr));
  temp_bytes = std::max(temp_bytes, want);
  DevBuf<int> d_rank, d_rn;   // the oversized components' nodes: flag, then number, of every node; the node of every number
  if (S.num_oversized_components) {
    if ((rc = d_sel.alloc((size_t)M)) || (rc = d_rank.alloc((size_t)N)) || (rc = d_rn.alloc((size_t)n))) return rc;
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, want, d_edge.p, d_eflag.p, d_sel.p, d_count.p, (int)M, nullptr));
    temp_bytes = std::max(temp_bytes, want);
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, want, ids, d_rank.p, d_rn.p, d_count.p, N, nullptr));
    temp_bytes = std::max(temp_bytes, want);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, want, d_rank.p, d_rank.p, N, nullptr));
    temp_bytes = std::max(temp_bytes, want);
  }
  if ((rc = d_temp.alloc(temp_bytes))) return rc;

  // the oversized components' edges in input order, between their nodes' numbers (ascending with the node ids)
  std::vector<uint64_t> replay_edges;
  int replay_nodes = 0;
  if (S.num_oversized_components) {
    k_tb_flag_nodes<<<grid_n, kThreads, 0, nullptr>>>(N, d_present.p, d_parent.p, d_size.p, max_len, d_rank.p);
    HIP_TRY(hipGetLastError());
    want = temp_bytes;
    HIP_TRY(hipcub::DeviceSelect::Flagged(d_temp.p, want, ids, d_rank.p, d_rn.p, d_count.p, N, nullptr));
    HIP_TRY(hipMemcpy(&replay_nodes, d_count.p, sizeof(int), hipMemcpyDeviceToHost));
    want = temp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp.p, want, d_rank.p, d_rank.p, N, nullptr));
    k_tb_flag_edges<<<grid_m, kThreads, 0, nullptr>>>(M, d_edge.p, d_parent.p, d_size.p, max_len, d_eflag.p);
    HIP_TRY(hipGetLastError());
    want = temp_bytes;
    HIP_TRY(hipcub::DeviceSelect::Flagged(d_temp.p, want, d_edge.p, d_eflag.p, d_sel.p, d_count.p, (int)M, nullptr));
    int selected = 0;
    HIP_TRY(hipMemcpy(&selected, d_count.p, sizeof(int), hipMemcpyDeviceToHost));
    k_tb_rank_edges<<<grid_of((size_t)selected, kThreads), kThreads, 0, nullptr>>>(selected, d_rank.p, d_sel.p);
    HIP_TRY(hipGetLastError());
    replay_edges.resize((size_t)selected);
    HIP_TRY(hipMemcpy(replay_edges.data(), d_sel.p, sizeof(uint64_t) * (size_t)selected, hipMemcpyDeviceToHost));
    S.num_replayed_correspondences = selected;
  }
  HIP_TRY(hipDeviceSynchronize());
  T.components_ms = ms_since(t_components);

  // the capped rule over those edges, on the host; the parts' roots back to the device, the sizes once more
  const auto t_replay = std::chrono::steady_clock::now();
  if (!replay_edges.empty()) {
    std::vector<int> root;
    replay_capped(replay_edges, replay_nodes, max_len, root);
    DevBuf<int> d_root;
    if ((rc = d_root.up(root.data(), root.size()))) return rc;
    k_tb_relabel<<<grid_of(root.size(), kThreads), kThreads, 0, nullptr>>>(replay_nodes, d_rn.p, d_root.p, d_parent.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemset(d_size.p, 0, sizeof(int) * (size_t)N));
    k_tb_sizes<<<grid_n, kThreads, 0, nullptr>>>(N, d_present.p, d_parent.p, d_size.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());   // d_root is freed at the end of this block
  }
  T.replay_ms = ms_since(t_replay);

  // nodes by (label, node id); the rules on the node count and on one feature per view; compaction
  const auto t_emit = std::chrono::steady_clock::now();
  DevBuf<int64_t> d_track_off;
  DevBuf<int32_t> d_obs_view, d_obs_feature, d_obs_track;
  if ((rc = d_track_off.alloc((size_t)n / 2 + 1)) || (rc = d_obs_view.alloc((size_t)n)) || (rc = d_obs_feature.alloc((size_t)n)) ||
      (rc = d_obs_track.alloc((size_t)n)))
    return rc;
  const int grid_nodes = grid_of((size_t)n, kThreads);
  want = temp_bytes;
  HIP_TRY(hipcub::DeviceSelect::Flagged(d_temp.p, want, ids, d_present.p, d_nodes.p, d_count.p, N, nullptr));
  k_tb_labels<<<grid_nodes, kThreads, 0, nullptr>>>(n, d_nodes.p, d_parent.p, d_labels.p);
  HIP_TRY(hipGetLastError());
  want = temp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp.p, want, d_labels.p, d_sl.p, d_nodes.p, d_sn.p, n, 0, label_bits, nullptr));
  k_tb_classify<<<grid_nodes, kThreads, 0, nullptr>>>(n, d_sl.p, d_sn.p, d_size.p, d_feat_off.p, num_views, min_len, d_view.p, d_flags.p,
                                                      d_counters.p);
  HIP_TRY(hipGetLastError());
  want = temp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp.p, want, d_flags.p, d_before.p, n, nullptr));
  k_tb_emit<<<grid_nodes, kThreads, 0, nullptr>>>(n, d_sn.p, d_view.p, d_flags.p, d_before.p, d_feat_off.p, d_track_off.p, d_obs_view.p,
                                                  d_obs_feature.p, d_obs_track.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  T.emit_ms = ms_since(t_emit);

  const auto t_download = std::chrono::steady_clock::now();
  uint64_t last_flags = 0, last_before = 0;
  HIP_TRY(hipMemcpy(&last_flags, d_flags.p + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&last_before, d_before.p + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost));
  S.num_small_components = (int64_t)counters[kSmall];
  S.num_inconsistent_features = (int64_t)counters[kInconsistent];
  S.num_tracks = (int64_t)((last_flags + last_before) >> 32);
  S.num_observations = (int64_t)(uint32_t)(last_flags + last_before);
  // every refusal lies behind: the tracks go straight into the caller's arrays
  const size_t no = (size_t)S.num_observations;
  if (S.num_tracks) HIP_TRY(hipMemcpy(track_off, d_track_off.p, sizeof(int64_t) * (size_t)S.num_tracks, hipMemcpyDeviceToHost));
  track_off[S.num_tracks] = S.num_observations;
  if (no) {
    HIP_TRY(hipMemcpy(obs_view, d_obs_view.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(obs_feature, d_obs_feature.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(obs_track, d_obs_track.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
  }
  if (stats) *stats = S;
  T.download_ms = ms_since(t_download);
  T.total_ms = ms_since(t_start);
  g_timings = T;
  return 0;
}
