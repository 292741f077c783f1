// ba_plan.hip -- everything that runs only inside theia_hip_ba_create: the flattening of a problem into wave tiles, the
// gather lists and the fused linearise + Schur plan (host threads, no device work but uploads), and the handle's allocations.
// The handle itself and the functions shared with the LM side are in ba_handle.h.
#include <atomic>
#include <cstdio>
#include <limits>
#include <map>
#include <mutex>
#include <new>

#include "ba_handle.h"
#include "ba_host_rules.h"
#include "ba_plan_stats.h"

namespace {

// std::vector without value-initialisation of trivially constructible elements (resize() leaves them uninitialised)
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U> struct rebind { using other = NoInitAlloc<U>; };
  template <class U, class... A>
  void construct(U* ptr, A&&... args) {
    if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(ptr)) U; else ::new (static_cast<void*>(ptr)) U(std::forward<A>(args)...);
  }
};

// A plain uninitialised array for the per-observation / per-track temporaries of create() that are written in full by the
// pass that fills them: value-initialising 15 MB of std::vectors was a millisecond of single-threaded memset per create().
template <class T>
struct RawArray {
  std::unique_ptr<T[]> p;
  explicit RawArray(size_t n) : p(new T[std::max<size_t>(1, n)]) {}
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  T* data() { return p.get(); }
};

// One stable counting pass on host threads: `to` = `from` ordered by digit (0 <= digit < nb), ties in input order.  Per-part
// histograms, offsets taken in (bucket, part) order; the result does not depend on the number of parts.
template <class T, class Digit>
void counting_pass(const T* from, T* to, int64_t n, int nb, Digit&& digit) {
  int parts = host_part_count(n, 32768);
  if (n < 393216 && !getenv("THEIA_HIP_HOST_CHUNK_MIN")) parts = 1;   // (two regions of the thread team cost more than a serial pass over a few hundred thousand entries)
  if ((int64_t)parts * nb > ((int64_t)1 << 24)) parts = 1;
  const int64_t per = (n + parts - 1) / parts;
  std::vector<int> head((size_t)parts * nb, 0);
  host_parts(parts, true, [&](int t) {
    int* hh = head.data() + (size_t)t * nb;
    for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); ++i) hh[digit(from[i])]++;
  });
  int run = 0;
  for (int b = 0; b < nb; ++b)
    for (int t = 0; t < parts; ++t) { int& c = head[(size_t)t * nb + b]; const int cnt = c; c = run; run += cnt; }
  host_parts(parts, true, [&](int t) {
    int* hh = head.data() + (size_t)t * nb;
    for (int64_t i = t * per; i < std::min<int64_t>(n, (t + 1) * per); ++i) to[hh[digit(from[i])]++] = from[i];
  });
}

__global__ void k_fill_value(double* x, size_t n, double v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = v;
}

// reduce_tiles configurations, uploaded once at create():
//   cfg 0 (linearize): {cost, gmax(max), invalid, notpd} -> rb.scal
//   cfg 1 (backsub)  : {cost, mcc, stepsq, xnormsq, invalid} -> scalB
//   cfg 2 (cost only): {cost, invalid} -> scalB
const int kCfgF2S[3][8] = {{SC_COST, SC_GMAX, SC_INVALID, SC_NOTPD, 0, 0, 0, 0},
                           {SB_COST, SB_MCC, SB_STEPSQ, SB_XNORMSQ, SB_INVALID, 0, 0, 0},
                           {SB_COST, SB_INVALID, 0, 0, 0, 0, 0, 0}};
const int kCfgMax[3][8] = {{0, 1, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};

#define UP(buf, vec) do { rc = h->buf.upload(vec, st); if (rc) return rc; } while (0)
#define AL(buf, cnt) do { rc = h->buf.alloc(cnt); if (rc) return rc; } while (0)
// Static gather lists of the Schur assembly without intrinsics (k_lin_obs / k_schur); see create().
// with_pairs = false (fused Schur assembly): only the per-camera observation lists the column-norm pass uses.
int build_gather_lists(theia_ba_handle_s* h, const int* ocam, const int* opt,
                       const std::vector<int>& l_obs, bool with_pairs = true) {
  int rc = 0;
  hipStream_t st = h->stream;
  // Static gather lists of the Schur assembly (k_schur_diag / k_schur_blocks):
  // per reduced camera its observations, per camera pair (ri > rj) the
  // (observation of ri, observation of rj) pairs of their common variable
  // tracks.  Tracks of the slow path (> 64 observations) assemble themselves.
  const int64_t nm = h->nobs_main;
  std::vector<char> is_long(l_obs.empty() ? 0 : nm, 0);
  for (int s2 : l_obs) is_long[s2] = 1;
  constexpr int kChunk = 2048;
  if (!with_pairs) {
    // Fused Schur assembly: only the cameras' observation lists are needed (column norms of the camera blocks,
    // k_colnorm_gather) -- a stable counting sort by reduced camera over a fixed partition of the observations, on host
    // threads, written into a pinned block.
    constexpr int kParts = 32;
    auto red_of = [&](int64_t s) { return (!is_long.empty() && is_long[s]) ? -1 : h->cam_red[ocam[s]]; };
    std::vector<std::vector<int>> fill(kParts, std::vector<int>(std::max(1, h->ncv), 0));
    const bool threaded = nm >= 262144;
    host_parts(kParts, threaded, [&](int k) {
      for (int64_t s = nm * k / kParts; s < nm * (k + 1) / kParts; ++s) { const int r = red_of(s); if (r >= 0) fill[k][r]++; }
    });
    std::vector<int> dbeg(h->ncv + 1, 0);
    for (int c = 0; c < h->ncv; ++c) {
      int at = dbeg[c];
      for (int k = 0; k < kParts; ++k) { const int cnt = fill[k][c]; fill[k][c] = at; at += cnt; }
      dbeg[c + 1] = at;
    }
    HBuf<int> sobs;
    const size_t nrec = (size_t)std::max(1, dbeg[h->ncv]);
    if (!sobs.resize(nrec, true)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %zu records failed", nrec);
    sobs[0] = 0;
    host_parts(kParts, threaded, [&](int k) {
      for (int64_t s = nm * k / kParts; s < nm * (k + 1) / kParts; ++s) { const int r = red_of(s); if (r >= 0) sobs[fill[k][r]++] = (int)s; }
    });
    std::vector<int> ditems;
    for (int c = 0; c < h->ncv; ++c) {
      const int nchunk = (dbeg[c + 1] - dbeg[c] + kChunk - 1) / kChunk;
      for (int k = 0; k < nchunk; ++k) {
        ditems.push_back(c); ditems.push_back(dbeg[c] + k * kChunk);
        ditems.push_back(std::min(dbeg[c + 1], dbeg[c] + (k + 1) * kChunk)); ditems.push_back(nchunk > 1 ? 1 : 0);
      }
    }
    h->n_diag_items = (int)ditems.size() / 4; h->n_blk_items = 0;
    if ((rc = h->slot_obs.upload(sobs.data(), nrec, st, sobs.pinned()))) return rc;
    UP(diag_items, ditems);   // pageable: synchronises the stream, the pinned block above is free after it
    return 0;
  }
  std::vector<int> red(nm);
  for (int64_t s = 0; s < nm; ++s) red[s] = (!is_long.empty() && is_long[s]) ? -1 : h->cam_red[ocam[s]];
  std::vector<int> dbeg(h->ncv + 1, 0);
  for (int64_t s = 0; s < nm; ++s) if (red[s] >= 0) dbeg[red[s] + 1]++;
  for (int c = 0; c < h->ncv; ++c) dbeg[c + 1] += dbeg[c];
  // records are stored camera-major: slot of observation s = its rank in its camera's list
  std::vector<int> cam_obs(nm, -1);   // = rec_slot
  {
    std::vector<int> f(dbeg.begin(), dbeg.end() - 1);
    for (int64_t s = 0; s < nm; ++s) if (red[s] >= 0) cam_obs[s] = f[red[s]]++;
  }
  std::vector<int> ditems;
  for (int c = 0; c < h->ncv; ++c) {
    const int nchunk = (dbeg[c + 1] - dbeg[c] + kChunk - 1) / kChunk;
    for (int k = 0; k < nchunk; ++k) {
      ditems.push_back(c); ditems.push_back(dbeg[c] + k * kChunk);
      ditems.push_back(std::min(dbeg[c + 1], dbeg[c] + (k + 1) * kChunk)); ditems.push_back(nchunk > 1 ? 1 : 0);
    }
  }
  // pairs, bucketed by row camera then sorted by column camera
  std::vector<int64_t> rbeg(h->ncv + 1, 0);
  auto for_each_pair = [&](auto&& fn) {
    for (int64_t s0 = 0; s0 < nm;) {
      int64_t s1 = s0 + 1;
      while (s1 < nm && opt[s1] == opt[s0]) ++s1;
      if ((is_long.empty() || !is_long[s0]) && !h->pt_const[opt[s0]])
        for (int64_t a = s0; a < s1; ++a) {
          if (red[a] < 0) continue;
          for (int64_t b = s0; b < s1; ++b)
            if (red[b] >= 0 && (red[a] > red[b] || (red[a] == red[b] && a != b))) fn((int)a, (int)b);
        }
      s0 = s1;
    }
  };
  for_each_pair([&](int a, int) { rbeg[red[a] + 1]++; });
  for (int c = 0; c < h->ncv; ++c) rbeg[c + 1] += rbeg[c];
  if (rbeg[h->ncv] > (int64_t)std::numeric_limits<int>::max() - 64)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "too many camera pairs for 32-bit pair lists");
  std::vector<int2> pairs(rbeg[h->ncv]);
  {
    std::vector<int64_t> f(rbeg.begin(), rbeg.end() - 1);
    for_each_pair([&](int a, int b) { pairs[f[red[a]]++] = make_int2(a, b); });
  }
  std::vector<int> bitems;
  // each row is ordered by (column camera, a, b).  The pairs of a row were generated in ascending (a, b)
  // (tracks are contiguous and visited in order), so a STABLE counting sort on the column camera is enough.
  {
    std::vector<int64_t> cnt(h->ncv + 1);
    std::vector<int2> tmp;
    for (int c = 0; c < h->ncv; ++c) {
      const int64_t b0 = rbeg[c], b1 = rbeg[c + 1];
      if (b1 - b0 < 2) continue;
      std::fill(cnt.begin(), cnt.end(), 0);
      for (int64_t q = b0; q < b1; ++q) cnt[red[pairs[q].y] + 1]++;
      for (int k = 0; k < h->ncv; ++k) cnt[k + 1] += cnt[k];
      tmp.assign(pairs.begin() + b0, pairs.begin() + b1);
      for (const int2& pr : tmp) pairs[b0 + cnt[red[pr.y]]++] = pr;
    }
  }
  for (int c = 0; c < h->ncv; ++c) {
    for (int64_t q = rbeg[c]; q < rbeg[c + 1];) {
      int64_t e = q + 1;
      const int rj = red[pairs[q].y];
      while (e < rbeg[c + 1] && red[pairs[e].y] == rj) ++e;
      const int nchunk = (int)((e - q + kChunk - 1) / kChunk);
      for (int k = 0; k < nchunk; ++k) {
        bitems.push_back(c); bitems.push_back(rj); bitems.push_back((int)(q + (int64_t)k * kChunk));
        bitems.push_back((int)std::min<int64_t>(e, q + (int64_t)(k + 1) * kChunk));
        bitems.push_back((nchunk > 1 || rj == c) ? 1 : 0);
      }
      q = e;
    }
  }
  // a camera that sees a track twice also has a (c, c) pair list: both kinds of items then ADD
  // into the diagonal block (they run in one launch, unordered)
  {
    std::vector<char> self(h->ncv, 0);
    for (size_t k = 0; k + 4 < bitems.size() + 1; k += 5) if (bitems[k] == bitems[k + 1]) self[bitems[k]] = 1;
    for (size_t k = 0; k + 3 < ditems.size() + 1; k += 4) if (self[ditems[k]]) ditems[k + 3] = 1;
  }
  // XCD-aware order: workgroup b runs on XCD b % 8 (observed dispatch order, a speed matter only).  All items whose
  // ROW camera is c are placed on XCD c % 8, so that camera's records are fetched into one L2 and re-used by its
  // block items and its diagonal item instead of being pulled into all eight.
  if (!getenv("THEIA_HIP_NO_XCD_ORDER")) {
    auto reorder = [&](std::vector<int>& items, int stride, int first_wg) {
      const int n = (int)items.size() / stride;
      std::vector<std::vector<int>> bucket(8);
      for (int k = 0; k < n; ++k) bucket[items[(size_t)k * stride] & 7].push_back(k);
      std::vector<size_t> head(8, 0);
      std::vector<int> out;
      out.reserve(items.size());
      for (int pos = 0; pos < n; ++pos) {
        int x = (first_wg + pos) & 7;
        if (head[x] >= bucket[x].size()) {   // that XCD's list is exhausted: take from the fullest one
          size_t best = 0;
          for (int y = 0; y < 8; ++y) { const size_t left = bucket[y].size() - head[y]; if (left > best) { best = left; x = y; } }
        }
        const int k = bucket[x][head[x]++];
        out.insert(out.end(), items.begin() + (size_t)k * stride, items.begin() + (size_t)(k + 1) * stride);
      }
      items.swap(out);
    };
    reorder(bitems, 5, 0);
    reorder(ditems, 4, (int)bitems.size() / 5);
  }
  h->n_diag_items = (int)ditems.size() / 4; h->n_blk_items = (int)bitems.size() / 5;
  for (auto& pr : pairs) { pr.x = cam_obs[pr.x]; pr.y = cam_obs[pr.y]; }
  {
    std::vector<int> sobs(std::max(1, dbeg[h->ncv]), 0);
    for (int64_t s2 = 0; s2 < nm; ++s2) if (cam_obs[s2] >= 0) sobs[cam_obs[s2]] = (int)s2;
    UP(slot_obs, sobs);
    std::vector<int> spt(sobs.size(), 0);
    for (int64_t s2 = 0; s2 < nm; ++s2) if (cam_obs[s2] >= 0) spt[cam_obs[s2]] = opt[s2];
    UP(slot_pt, spt);
  }
  UP(diag_items, ditems); UP(cam_obs, cam_obs); UP(blk_items, bitems); UP(blk_pairs, pairs);
  AL(rec, (size_t)std::max(1, dbeg[h->ncv]) * (6 * h->pd + 14));
  return 0;
}

// The gather lists when intrinsics are optimised (k_lin_obs_intr / k_schur_intr); see create().
int build_gather_lists_intr(theia_ba_handle_s* h, const theia_ba_problem* p, const int* ocam,
                            const int* opt, const std::vector<int>& l_obs) {
  const bool itiming = getenv("THEIA_HIP_CREATE_TIMING") != nullptr;
  double it0 = now_s();
  auto itick = [&](const char* what) {
    if (!itiming) return;
    const double t = now_s();
    fprintf(stderr, "theia_hip create:     intrinsics lists: %-24s %8.2f ms\n", what, 1e3 * (t - it0));
    it0 = t;
  };
  int rc = 0;
  hipStream_t st = h->stream;
  // Gather lists with intrinsics (k_lin_obs_intr / k_schur_intr): records for every observation whose camera OR
  // intrinsics group is variable, stored (group, camera)-major; item = {type, row0, col0, beg, end, flags}.
  enum { IT_CC = 0, IT_CG = 1, IT_GG0 = 2, IT_GG1 = 3, IT_CD = 4, IT_CGD = 5, IT_GD0 = 6, IT_GD1 = 7, IT_GV = 8 };
  const int64_t nm = h->nobs_main;
  constexpr int kChunk = 2048;
  std::vector<int> red(nm), grd(nm);
  for (int64_t s = 0; s < nm; ++s) { red[s] = h->cam_red[ocam[s]]; grd[s] = h->grp_red[p->cam_group[ocam[s]]]; }
  for (int s2 : l_obs) { red[s2] = -1; grd[s2] = -1; }   // tracks of the slow path (k_long_*) assemble themselves
  // slots: sort the observations that need a record by (group, camera)
  std::vector<int> order;
  for (int64_t s = 0; s < nm; ++s) if (red[s] >= 0 || grd[s] >= 0) order.push_back((int)s);
  {   // stable sort by (group, camera): two counting passes, camera first (keys start at -1)
    std::vector<int> tmp(order.size());
    for (int pass = 0; pass < 2; ++pass) {
      const std::vector<int>& key = pass == 0 ? red : grd;
      std::vector<size_t> cnt((size_t)(pass == 0 ? h->ncv : h->ngv) + 2, 0);
      for (int x : order) cnt[(size_t)(key[x] + 1) + 1]++;
      for (size_t k = 0; k + 1 < cnt.size(); ++k) cnt[k + 1] += cnt[k];
      for (int x : order) tmp[cnt[(size_t)(key[x] + 1)]++] = x;
      order.swap(tmp);
    }
  }
  std::vector<int> slot(nm, -1);
  for (size_t k = 0; k < order.size(); ++k) slot[order[k]] = (int)k;
  itick("record order");
  std::vector<int> items;
  auto push_item = [&](int type, int row0, int col0, int64_t beg, int64_t end, int flags) {
    const int nchunk = (int)((end - beg + kChunk - 1) / kChunk);
    for (int k = 0; k < nchunk; ++k) {
      items.push_back(type); items.push_back(row0); items.push_back(col0);
      items.push_back((int)(beg + (int64_t)k * kChunk)); items.push_back((int)std::min<int64_t>(end, beg + (int64_t)(k + 1) * kChunk));
      items.push_back(flags | (nchunk > 1 ? 1 : 0));
    }
  };
  // ---- pair lists: entries (key, slot a, slot b) sorted by key; one item (or two halves) per key
  // Camera x camera blocks take every ordered pair of observations of a track.  For the blocks with an intrinsics group
  // on one or both sides, a track that sees few variable groups is represented by the SUMS of its observations'
  // intrinsics fields, one per group (pseudo-records behind the real ones, written by k_lin_obs_intr from segmented wave sums):
  // Sum_b T_a WI_b^T = T_a (Sum_b WI_b)^T, so the track gives L (observation, sum) pairs and one (sum, sum) pair instead
  // of 2 L (L - 1) ordered pairs.  The sum includes b == a, so the per-observation items leave that term out for the
  // observations of such a track (slot_in_sum).  Tracks that see several variable groups keep their explicit pairs.
  // THEIA_HIP_INTR_PAIRS=1 keeps the lists of the first version (no sums).
  struct PairE { uint64_t key; int a, b; };
  const bool track_sums = !getenv("THEIA_HIP_INTR_PAIRS");
  const int nslots = (int)order.size();
  // The tracks are walked twice on host threads, in a fixed number of ranges of consecutive tracks: the first walk counts a
  // range's entries and pseudo-records, the second writes them at the offsets the counts give -- the lists come out in track
  // order whatever the number of threads (one thread pushing ~20 M entries into growing vectors took 145 ms at 1000 views).
  std::vector<int64_t> tbeg;   // first sorted observation of every track with non-fixed observations, then nm
  for (int64_t s0 = 0; s0 < nm;) {
    int64_t s1 = s0 + 1;
    while (s1 < nm && opt[s1] == opt[s0]) ++s1;
    tbeg.push_back(s0);
    s0 = s1;
  }
  tbeg.push_back(nm);
  const int64_t ntrk = (int64_t)tbeg.size() - 1;
  constexpr int kTrackParts = 64;
  struct PartCount { size_t cc = 0, cg = 0, gg = 0; int sums = 0; };
  std::vector<PartCount> pc(kTrackParts + 1);
  std::vector<int> pt_sum(track_sums ? h->np : 0, -1);   // pseudo-record slot of a track, -1 = none
  std::vector<uint8_t> slot_sum(track_sums ? std::max(1, nslots) : 0, 0);
  std::vector<uint8_t> pt_cnt(track_sums ? h->np : 0, 0);   // number of summed groups of a track
  std::vector<int> sum_group;                               // group of a pseudo-record
  PairE* ccp = nullptr; PairE* cgp = nullptr; PairE* ggp = nullptr;
  // one track: sink_cc / sink_cg / sink_gg receive its entries in the order of the one-thread loop; `ps` is its first pseudo-record
  auto walk_track = [&](int64_t s0, int64_t s1, int ps, bool write, PartCount& n) {
    if (h->pt_const[opt[s0]]) return;
    // the track's variable groups in order of first appearance (long tracks carry -1 everywhere: none).  A track is
    // summed per group when that shortens its lists: one group, or fewer groups (at most kMaxSumGroups) than
    // observations of variable groups
    constexpr int kMaxSumGroups = 4;
    int tgs[kMaxSumGroups], ntg = 0, lg = 0;
    bool many = false;
    for (int64_t b2 = s0; b2 < s1; ++b2) {
      if (grd[b2] < 0) continue;
      ++lg;
      bool seen = false;
      for (int k = 0; k < ntg; ++k) seen |= tgs[k] == grd[b2];
      if (seen) continue;
      if (ntg == kMaxSumGroups) { many = true; break; }
      tgs[ntg++] = grd[b2];
    }
    const bool sum_mode = track_sums && !many && ntg >= 1 && (ntg == 1 || ntg < lg);
    auto put = [&](PairE* base, size_t& at, uint64_t key, int x, int y) { if (write) base[at] = PairE{key, x, y}; ++at; };
    for (int64_t x = s0; x < s1; ++x)
      for (int64_t y = s0; y < s1; ++y) {
        if (x == y) continue;
        if (red[x] >= 0 && red[y] >= 0 && red[x] >= red[y]) put(ccp, n.cc, ((uint64_t)red[x] << 32) | (uint32_t)red[y], slot[x], slot[y]);
        if (sum_mode) continue;
        if (red[x] >= 0 && grd[y] >= 0) put(cgp, n.cg, ((uint64_t)red[x] << 32) | (uint32_t)grd[y], slot[x], slot[y]);
        if (grd[x] >= 0 && grd[y] >= 0 && grd[x] >= grd[y]) put(ggp, n.gg, ((uint64_t)grd[x] << 32) | (uint32_t)grd[y], slot[x], slot[y]);
      }
    if (sum_mode) {
      const int my = ps + n.sums;   // pseudo-records my .. my + ntg - 1, one per group
      if (write) {
        pt_sum[opt[s0]] = my; pt_cnt[opt[s0]] = (uint8_t)ntg;
        for (int k = 0; k < ntg; ++k) sum_group[(size_t)(my - nslots + k)] = tgs[k];
      }
      for (int64_t x = s0; x < s1; ++x) {
        if (write && slot[x] >= 0) slot_sum[slot[x]] = 1;
        if (red[x] >= 0)
          for (int k = 0; k < ntg; ++k) put(cgp, n.cg, ((uint64_t)red[x] << 32) | (uint32_t)tgs[k], slot[x], my + k);
      }
      for (int k = 0; k < ntg; ++k)
        for (int k2 = 0; k2 < ntg; ++k2)
          if (tgs[k] >= tgs[k2]) put(ggp, n.gg, ((uint64_t)tgs[k] << 32) | (uint32_t)tgs[k2], my + k, my + k2);
      n.sums += ntg;
    }
  };
  auto part_range = [&](int k, int64_t* t0, int64_t* t1) { *t0 = ntrk * k / kTrackParts; *t1 = ntrk * (k + 1) / kTrackParts; };
  host_parts(kTrackParts, ntrk >= 4096, [&](int k) {
    int64_t t0, t1; part_range(k, &t0, &t1);
    PartCount n;
    for (int64_t t = t0; t < t1; ++t) walk_track(tbeg[t], tbeg[t + 1], 0, false, n);
    pc[k + 1] = n;
  });
  for (int k = 0; k < kTrackParts; ++k) { pc[k + 1].cc += pc[k].cc; pc[k + 1].cg += pc[k].cg; pc[k + 1].gg += pc[k].gg; pc[k + 1].sums += pc[k].sums; }
  const int nsums = pc[kTrackParts].sums;
  std::vector<PairE, NoInitAlloc<PairE>> cc, cg, gg;   // (resize() does not touch the 100s of MB)
  {
    cc.resize(pc[kTrackParts].cc); cg.resize(pc[kTrackParts].cg); gg.resize(pc[kTrackParts].gg);
    sum_group.assign((size_t)nsums, 0);
    ccp = cc.data(); cgp = cg.data(); ggp = gg.data();
  }
  host_parts(kTrackParts, ntrk >= 4096, [&](int k) {
    int64_t t0, t1; part_range(k, &t0, &t1);
    PartCount n = pc[k];
    for (int64_t t = t0; t < t1; ++t) walk_track(tbeg[t], tbeg[t + 1], nslots, true, n);
  });
  itick("pair entries");
  // (the pair list is written into a block of the pinned host cache and uploaded from there)
  HBuf<int2> pairs;
  size_t npairs = 0;
  if (!pairs.resize(std::max<size_t>(1, cc.size() + cg.size() + gg.size()), true))
    return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %zu pairs failed", cc.size() + cg.size() + gg.size());
  // entries are generated in ascending (a, b): two stable counting passes (low, then high half of the key)
  // order them by (key, a, b) without a comparison sort
  const size_t nbucket = (size_t)std::max(h->ncv, h->ngv) + 2;
  // (one uninitialised scratch array for the three lists: a value-initialised vector of the 10 - 25 M entries was a 100+ MB memset,
  // and a fresh one per list two more rounds of page faults)
  RawArray<PairE> tmp_raw(std::max(cc.size(), std::max(cg.size(), gg.size())));
  auto emit_pairs = [&](auto& v, auto&& per_key) {
    const size_t nv = v.size();
    PairE* a = v.data();
    PairE* b = tmp_raw.data();
    {   // each pass over a fixed 32-way partition of the entries with per-part histograms, on host threads (stable)
      constexpr int kParts = 32;
      const bool threaded = nv >= 262144;
      std::vector<std::vector<size_t>> cnt(kParts, std::vector<size_t>(nbucket));
      for (int pass = 0; pass < 2; ++pass) {
        const int sh = pass == 0 ? 0 : 32;
        host_parts(kParts, threaded, [&](int k) {
          std::fill(cnt[k].begin(), cnt[k].end(), 0);
          for (size_t i = nv * k / kParts; i < nv * (k + 1) / kParts; ++i) cnt[k][(size_t)((a[i].key >> sh) & 0xffffffffu)]++;
        });
        size_t at = 0;
        for (size_t bk = 0; bk < nbucket; ++bk)
          for (int k = 0; k < kParts; ++k) { const size_t c = cnt[k][bk]; cnt[k][bk] = at; at += c; }
        host_parts(kParts, threaded, [&](int k) {
          for (size_t i = nv * k / kParts; i < nv * (k + 1) / kParts; ++i) b[cnt[k][(size_t)((a[i].key >> sh) & 0xffffffffu)]++] = a[i];
        });
        std::swap(a, b);
      }
    }
    // (two passes: the sorted entries are back in v) -- the pair list is their (a, b) columns, copied on host threads; the key
    // boundaries come from one scan
    const int64_t base = (int64_t)npairs;
    npairs += nv;
    int2* out = pairs.data() + base;
    constexpr int kScanParts = 32;
    std::vector<std::vector<size_t>> starts(kScanParts);   // first entries of the keys, per range of the scan
    host_parts(kScanParts, nv >= 262144, [&](int k) {
      for (size_t i = nv * k / kScanParts; i < nv * (k + 1) / kScanParts; ++i) {
        out[i] = make_int2(a[i].a, a[i].b);
        if (i == 0 || a[i].key != a[i - 1].key) starts[k].push_back(i);
      }
    });
    std::vector<size_t> first;
    for (const auto& v2 : starts) first.insert(first.end(), v2.begin(), v2.end());
    first.push_back(nv);
    for (size_t k = 0; k + 1 < first.size(); ++k) {
      const size_t q = first[k], e = first[k + 1];
      per_key((int)(a[q].key >> 32), (int)(a[q].key & 0xffffffffu), base + (int64_t)q, base + (int64_t)e);
    }
  };
  // cameras seen twice by a track give (c, c) lists: the camera block is then fed by two kinds of items
  std::vector<char> self(h->ncv, 0);
  for (const PairE& e : cc) if ((e.key >> 32) == (e.key & 0xffffffffu)) self[e.key >> 32] = 1;
  emit_pairs(cc, [&](int ra, int rb, int64_t beg, int64_t end) {
    push_item(IT_CC, h->ni + 6 * ra, h->ni + 6 * rb, beg, end, ra == rb ? 3 : 0);
  });
  emit_pairs(cg, [&](int ra, int gb, int64_t beg, int64_t end) { push_item(IT_CG, h->ni + 6 * ra, 10 * gb, beg, end, 1); });
  const bool compact = h->intr_rows == 4;   // four compact intrinsics rows: one GG / GD item instead of the 4 + 6 split
  emit_pairs(gg, [&](int ga, int gb, int64_t beg, int64_t end) {
    push_item(IT_GG0, 10 * ga, 10 * gb, beg, end, 1 | (ga == gb ? 2 : 0));
    if (!compact) push_item(IT_GG1, 10 * ga, 10 * gb, beg, end, 1 | (ga == gb ? 2 : 0));
  });
  // (the CG / GG targets also receive the per-observation diagonal items below: always atomic)
  itick("sorted pair lists");
  if (npairs > (size_t)std::numeric_limits<int>::max() - 64)
    return set_error(THEIA_HIP_ERR_UNSUPPORTED, "too many observation pairs for 32-bit pair lists");
  // ---- per-observation (diagonal) items over contiguous slot ranges
  for (size_t q = 0; q < order.size();) {   // per camera (inside its group)
    size_t e = q + 1;
    while (e < order.size() && red[order[e]] == red[order[q]] && grd[order[e]] == grd[order[q]]) ++e;
    const int rc = red[order[q]], gr = grd[order[q]];
    if (rc >= 0) {
      push_item(IT_CD, h->ni + 6 * rc, h->ni + 6 * rc, (int64_t)q, (int64_t)e, self[rc] ? 1 : 0);
      if (gr >= 0) push_item(IT_CGD, h->ni + 6 * rc, 10 * gr, (int64_t)q, (int64_t)e, 1);
    }
    q = e;
  }
  for (size_t q = 0; q < order.size();) {   // per group
    size_t e = q + 1;
    while (e < order.size() && grd[order[e]] == grd[order[q]]) ++e;
    const int gr = grd[order[q]];
    if (gr >= 0) {
      push_item(IT_GD0, 10 * gr, 10 * gr, (int64_t)q, (int64_t)e, 1);
      if (!compact) push_item(IT_GD1, 10 * gr, 10 * gr, (int64_t)q, (int64_t)e, 1);
      push_item(IT_GV, 10 * gr, 10 * gr, (int64_t)q, (int64_t)e, 0);
    }
    q = e;
  }
  h->n_diag_items = 0; h->n_blk_items = (int)items.size() / 6;
  {
    std::vector<int> sobs(order.begin(), order.end());
    if (sobs.empty()) sobs.push_back(0);
    UP(slot_obs, sobs);
  }
  UP(cam_obs, slot); UP(blk_items, items);
  if ((rc = h->blk_pairs.upload(pairs.data(), std::max<size_t>(1, npairs), st, pairs.pinned()))) return rc;
  itick("items + uploads");
  h->n_trk_sums = nsums;
  h->sum_base = nslots;
  if (nsums) { UP(pt_sum_slot, pt_sum); UP(slot_in_sum, slot_sum); UP(pt_sum_cnt, pt_cnt); UP(sum_group, sum_group); }
  AL(rec, (std::max<size_t>(1, order.size()) + (size_t)h->n_trk_sums) * (12 * h->pd + 20 + 2 * h->intr_rows * h->pd + 3 * h->intr_rows));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Plan of the fused linearise + Schur kernel (ba_fused.hip): wave tiles, runs, local camera tables, target
// blocks, and the per-S-block lists of partial sums.  Replaces build_tiles() for the main tiles.
//   off    : [np + 1] offsets of the tracks (by rank) into the sorted observation arrays
//   sred   : [nobs_main] reduced camera index of a sorted observation (-1 = constant camera)
//   skey   : [np] ordering key of a track rank (its first variable camera)
// Tracks that do not fit the fused kernel (more than 64 observations, more than kFusedMaxCams variable cameras,
// a camera seen twice) go to the per-observation slow path (k_long_*), like the > 64 ones before.
// local cameras a run of the fused plan may hold: its target blocks (pairs, diagonal included) times the lanes per block fit the
// 256 threads of a workgroup -- 22 cameras / 253 blocks of one lane; compound blocks of width bw: three rows per lane
inline int fused_run_cameras(int bw) {
  if (bw == 0) return kFusedMaxCams;
  if (bw == 9) return kFusedMaxCamsIntr;   // 78 blocks x 3 lanes
  if (bw == 10) return 10;                 // 55 x 4
  return 10;                               // 13 / 16 rows: 55 x 4
}
// lanes of a target block (ba_fused_intr.hip: lanes_per_target): three rows per lane up to width 10, four at 13
inline int fused_lanes_per_target(int bw) { return bw == 0 ? 1 : (bw <= 10 ? (bw + 2) / 3 : (bw + 3) / 4); }

// What one more run costs k_lin_schur, in wave steps of phase S (the unit of ba_plan_stats.h): run setup is 4 % and the slice
// combination with its stores 11 % of the kernel where phase S is 38 %, over the 2102 runs and 339 k issued
// steps of the C4 plan: 0.15 / 0.38 x 339 k / 2102 = 64.
constexpr double kFusedRunCostSteps = 64.0;

// runs whose dealt slot rows differed from the closed form their shape was chosen on (shape_slices: they keep equal slices);
// THEIA_HIP_CREATE_TIMING prints it, zero on every plan measured
inline std::atomic<long long>& shape_mismatches() { static std::atomic<long long> n{0}; return n; }

struct FusedHost {
  std::vector<FusedRun> runs;
  std::vector<int> cams, stage, tile_trk_end, sum_items, sum_src;
  std::vector<unsigned short> tgts;
  std::vector<uint8_t> obs_lc, obs_tl;
  std::vector<uint8_t> tile_adj;   // [nt][nt] 64-wide tiles of S coupled by a variable track (the K3 plan's input)
  size_t part_doubles = 0;
};
// One contiguous range [q_begin, q_end) of track ranks -> the tiles / runs / long tracks of that range, with tile, camera-table,
// target and partial-sum offsets relative to the segment (merge_fused_segments rebases them).  obs_lc / obs_tl are indexed
// by observation: segments write disjoint parts of the shared arrays.
struct FusedSegment {
  std::vector<int> tstart, tcount, tkey, l_obs, l_slot, l_start, l_pt;
  FusedHost fp;
};
void build_fused_segment(const theia_ba_handle_s* h, const std::vector<int64_t>& off, const std::vector<int>& porder,
                         const int* sred, const int* ocam, const std::vector<int>& skey, int q_begin, int q_end,
                         uint8_t* obs_lc, uint8_t* obs_tl, FusedSegment& seg) {
  std::vector<int>& tstart = seg.tstart; std::vector<int>& tcount = seg.tcount; std::vector<int>& tkey = seg.tkey;
  std::vector<int>& l_obs = seg.l_obs; std::vector<int>& l_slot = seg.l_slot; std::vector<int>& l_start = seg.l_start;
  std::vector<int>& l_pt = seg.l_pt;
  FusedHost& fp = seg.fp;
  const int64_t nm = h->nobs_main;
  const int tps = fused_tiles_per_subchunk(h->pd);
  // geometry of the consumer lanes: lanes per target block, rows per local camera, partial-sum doubles (ba_fused.hip:
  // one lane per 6 x 6 block; ba_fused_intr.hip: 3 or 4 lanes per compound block, stored 10 x 10)
  const int bw = h->fused_bw;
  const size_t lanes_tgt = bw == 0 ? 1 : (size_t)fused_lanes_per_target(bw), rows_cam = bw == 0 ? 6 : (size_t)bw;
  const size_t part_tgt = bw == 0 ? 36 : (size_t)bw * bw, part_cam = bw == 0 ? 18 : (size_t)3 * bw;   // compound blocks: BW x BW per target, BW x 3 per camera
  const int max_cams = fused_run_cameras(bw);
  const size_t max_tgts = bw == 0 ? 253 : 256 / lanes_tgt;
  // track slices per consumer wave for a run of ntgt target blocks over W cameras (0 = needs more than one wave)
  auto packing = [&](size_t ntgt, size_t W) -> int {
    if (lanes_tgt * ntgt > 64 || rows_cam * W > 64) return 0;
    static const int cand[6] = {10, 6, 4, 3, 2, 1};
    for (int c : cand) if ((size_t)(64 / c) >= lanes_tgt * ntgt) return c;
    return 1;
  };
  const char* rm = getenv("THEIA_HIP_FUSED_RUN_OBS");
  const int64_t run_max = rm ? std::max(64, atoi(rm)) : std::max<int64_t>(256, std::min<int64_t>(2048, nm / 600));   // 3.0 M observations, round-5 kernel (cameras staged per run, queue popped one run ahead): 2048 0.364 ms, 1664 0.365, 1344 0.372, 1024 0.39 (round 4: 1344)
  // current tile / run
  int64_t t_start = 0, t_len = 0;
  int t_tracks = 0, sc_tracks = 0;
  int run_tile0 = 0, run_ntiles = 0, run_key0 = -1;
  int64_t run_obs = 0;
  // cameras / co-visible camera pairs of the open run: membership through per-run stamps (a sorted-set union per track
  // cost 64 ms at 500k tracks), the lists are sorted once when the run closes
  std::vector<int> run_cams;           // unique, sorted by finalize_run
  std::vector<int64_t> run_pairs;      // unique keys hi * 2^32 | lo of co-visible reduced cameras (hi >= lo), sorted by finalize_run
  std::vector<int> tc;
  std::vector<int64_t> tp;
  int serial = 1;
  // camera sets that joined the open run (a small direct-mapped table, entries of other runs are stale by their stamp): a track
  // with one of them brings nothing new -- at C4 a run sees three to six distinct sets, and probing a track's <= 55 pairs twice
  // was most of this function
  struct SeenSet { int stamp = 0, n = 0; int cams[kFusedMaxCams]; };
  constexpr int kSeenSets = 64;
  std::vector<SeenSet> seen_sets(kSeenSets);
  std::vector<int> cam_stamp((size_t)std::max(1, h->ncp), 0);
  std::vector<uint8_t> cam_local((size_t)std::max(1, h->ncp), 0);   // camera -> index in the closing run's sorted table
  // CONSTANT cameras the open run's tracks see (the fused kernels stage their blocks in LDS behind the local cameras'), in order
  // of appearance: obs_lc = 0x80 | index
  const int max_const = bw == 0 ? kFusedMaxConst : kFusedMaxConstIntr;
  static_assert(kFusedMaxConst <= 0x7f && kFusedMaxConstIntr <= 0x7f, "obs_lc keeps the constant-camera index in seven bits");
  std::vector<int> run_ccams, tcc;
  std::vector<int> ccam_stamp((size_t)std::max(1, h->nc), 0);
  std::vector<uint8_t> ccam_local((size_t)std::max(1, h->nc), 0);
  constexpr int kPairSlots = 2048;     // > 4 x 253
  std::vector<int64_t> pair_key(kPairSlots, 0);
  std::vector<int> pair_stamp(kPairSlots, 0);
  auto pair_slot = [&](int64_t key) -> int {   // slot holding `key` in this run, or the free slot where it would go
    unsigned hsh = ((unsigned)(key >> 32) * 0x9E3779B1u) ^ ((unsigned)key * 0x85EBCA77u);
    int sl = (int)(hsh >> 21) & (kPairSlots - 1);
    while (pair_stamp[sl] == serial && pair_key[sl] != key) sl = (sl + 1) & (kPairSlots - 1);
    return sl;
  };
  const int adj_nt = (h->n + 63) / 64;
  fp.tile_adj.assign((size_t)adj_nt * adj_nt, 0);
  std::vector<int> tl;
  auto mark_tiles = [&](int q) {   // tile co-visibility of a variable track (tc: its variable cameras, ascending)
    if (h->pt_const[porder[q]]) return;
    tl.clear();
    for (int pcam : tc) {
      const int rcam = h->cam_red[h->part_cam[pcam]];   // (participating camera -> reduced camera; constant: no rows in S)
      if (rcam < 0) continue;
      const int s0 = h->ni + 6 * rcam;
      if (tl.empty() || tl.back() != s0 / 64) tl.push_back(s0 / 64);
      if ((s0 + 5) / 64 != s0 / 64) tl.push_back((s0 + 5) / 64);
    }
    for (int a : tl) for (int b : tl) fp.tile_adj[(size_t)a * adj_nt + b] = 1;
  };

  auto close_tile = [&](int q_end) {
    if (!t_len) return;
    tstart.push_back((int)t_start); tcount.push_back((int)t_len); tkey.push_back(run_key0 < 0 ? 0 : run_key0);
    (void)q_end;
    fp.tile_trk_end.push_back(sc_tracks);
    run_ntiles++;
    t_len = 0; t_tracks = 0;
  };
  // the tracks of the open run: first observation, length, highest variable camera, wave tile, targets it needs (shape_slices)
  struct RunTrack { int s0, cmax, tile; uint8_t len, need; };
  std::vector<RunTrack> run_trk;
  int run_kmin = 64;   // fewest variable cameras of a track of the open run
  std::vector<int> need_desc, sc_gt, sc_n, sc_first, slot_of, sc_slots, by_need;
  const bool unequal_slices = !getenv("THEIA_HIP_FUSED_EQUAL_SLICES");   // (the switch: A/B measurements; read per plan)
  // Unequal track slices (k_lin_schur, one wave per slice row: G == 1).  The targets of a run are sorted by (la, lb), la >= lb,
  // so a track whose highest local camera is m has all its pairs among the first need = 1 + index of (m, m) targets: a slice
  // that owns only a PREFIX of the targets serves every track with need <= its width.  Slice 0 keeps all ntgt targets, the
  // others share the remaining lanes, and the tracks of a sub-chunk are dealt to the slots (row, slice) they fit -- most
  // demanding first, to the emptiest slice -- instead of in order.  The shape is the one with the fewest slot rows (= wave steps
  // that run the pair products, ba_plan_stats.h) over the run's sub-chunks; equal slices stay unless it saves 1/16 of them.
  // A pure function of the run's tracks in plan order.
  auto shape_slices = [&](FusedRun& r) {
    const int PS0 = r.gp >> 8, ntrk = (int)run_trk.size(), nsc = (run_ntiles + tps - 1) / tps;
    // (a track of k cameras needs its own k (k + 1) / 2 pairs at least: where not even the shortest fits beside slice 0 -- the
    // long-track runs of C4 -- nothing below is looked at; a run of a few tracks has no rows to save)
    if (r.ntgt < 2 || ntrk < 8 || r.ntgt + std::max(1, run_kmin * (run_kmin + 1) / 2) > 64) return;
    int hist[66] = {0}, diag_at[kFusedMaxCams] = {0};   // diag_at[m]: the targets up to and including (m, m)
    for (int k = 0; k < r.ntgt; ++k) { const unsigned us = fp.tgts[(size_t)r.tgt_off + k]; if ((us & 0xff) == (us >> 8)) diag_at[us & 0xff] = k + 1; }
    int least = 64;
    for (RunTrack& t : run_trk) { t.need = (uint8_t)(t.cmax >= 0 ? diag_at[cam_local[t.cmax]] : 0); hist[t.need]++; least = std::min<int>(least, t.need); }
    if (r.ntgt + std::max(1, least) > 64) return;   // (the same with the needs themselves)
    const size_t NW = (size_t)r.ntgt + 1;           // needs are 0 .. ntgt
    need_desc.clear();   // the run's needs, descending
    for (int v = 64; v >= 0; --v) need_desc.insert(need_desc.end(), (size_t)hist[v], v);
    sc_gt.assign((size_t)nsc * NW, 0); sc_n.assign((size_t)nsc, 0); sc_first.assign((size_t)nsc + 1, ntrk);
    for (int i = ntrk - 1; i >= 0; --i) {   // (tracks joined in tile order: a sub-chunk's tracks are one range of run_trk)
      const int sc = (run_trk[i].tile - run_tile0) / tps;
      sc_first[sc] = i; sc_n[sc]++;
      if (run_trk[i].need > 0) sc_gt[(size_t)sc * NW + run_trk[i].need - 1]++;
    }
    for (int sc = 0; sc < nsc; ++sc)   // sc_gt[sc][v] = tracks of the sub-chunk with need > v
      for (int v = r.ntgt - 2; v >= 0; --v) sc_gt[(size_t)sc * NW + v] += sc_gt[(size_t)sc * NW + v + 1];
    for (int sc = nsc - 1; sc >= 0; --sc) if (sc_n[sc] == 0) sc_first[sc] = sc_first[sc + 1];
    // slot rows of a shape over the sub-chunks (-1: a sub-chunk would need more than the 128 slots of the kernel's tables)
    auto rows_of = [&](const int* wid, int p) -> long long {
      long long rows = 0;
      for (int sc = 0; sc < nsc; ++sc) {
        int rs = (sc_n[sc] + p - 1) / p;
        for (int j = 1; j < p; ++j) {
          const int over = sc_gt[(size_t)sc * NW + wid[j]];   // these tracks need a slice wider than wid[j]
          if (!over) continue;
          int wider = 0;
          while (wider < j && wid[wider] > wid[j]) ++wider;
          rs = std::max(rs, (over + wider - 1) / std::max(1, wider));
        }
        if (rs * p > kFusedTileTracks * tps) return -1;
        rows += rs;
      }
      return rows;
    };
    int eq[kFusedMaxSlices];
    for (int j = 0; j < PS0; ++j) eq[j] = r.ntgt;
    const long long rows_eq = rows_of(eq, PS0);
    // candidates: for a number of rows R of the whole run, slice j must take the tracks ranked j R .. (j + 1) R - 1 by need
    int best[kFusedMaxSlices], bestp = 0, last[kFusedMaxSlices], lastp = 0, tried = 0;
    long long best_rows = -1;
    for (int R = (ntrk + kFusedMaxSlices - 1) / kFusedMaxSlices; R < ntrk && tried < 2; ++R) {
      int wid[kFusedMaxSlices], p = 0, sum = 0;
      for (int j = 0; j * R < ntrk && p < kFusedMaxSlices && sum <= 64; ++j) {
        const int w = j == 0 ? r.ntgt : need_desc[(size_t)j * R];
        if (w == 0) break;   // (tracks without a variable camera fit any slice)
        wid[p++] = w; sum += w;
      }
      if (sum > 64 || p < 2) continue;
      if (p == lastp && std::equal(wid, wid + p, last)) continue;
      std::copy(wid, wid + p, last); lastp = p; ++tried;
      // (and the same with what is left of the wave given to the narrow slices, next need up: slack for the sub-chunks' mix)
      for (int variant = 0; variant < 2; ++variant) {
        if (variant)
          for (int j = p - 1; j >= 1; --j) {
            int up = wid[j] + 1;
            while (up <= wid[j - 1] && !hist[up]) ++up;
            if (up <= wid[j - 1] && sum - wid[j] + up <= 64) { sum += up - wid[j]; wid[j] = up; }
          }
        const long long rows = rows_of(wid, p);
        if (rows >= 0 && (best_rows < 0 || rows < best_rows)) { best_rows = rows; bestp = p; std::copy(wid, wid + p, best); }
      }
    }
    if (best_rows < 0 || rows_eq < 0 || best_rows * 16 > rows_eq * 15) return;
    // deal the tracks of every sub-chunk to their slots
    slot_of.assign((size_t)ntrk, 0); sc_slots.assign((size_t)nsc, 0);
    uint8_t fits_of[66];   // slices wide enough for a need (widths do not increase)
    for (int v = 0, fits = bestp; v <= r.ntgt; ++v) { while (fits > 0 && best[fits - 1] < v) --fits; fits_of[v] = (uint8_t)fits; }
    long long dealt_rows = 0;
    for (int sc = 0; sc < nsc; ++sc) {
      {   // the sub-chunk's tracks by need, descending, ties in plan order (one counting pass)
        int at[66];
        for (int v = 0; v <= r.ntgt; ++v) at[v] = sc_gt[(size_t)sc * NW + v];   // the tracks with need > v come first
        by_need.assign((size_t)(sc_first[sc + 1] - sc_first[sc]), 0);
        for (int i = sc_first[sc]; i < sc_first[sc + 1]; ++i) by_need[(size_t)at[run_trk[i].need]++] = i;
      }
      int fill[kFusedMaxSlices] = {0};
      for (int i : by_need) {
        const int fits = fits_of[run_trk[i].need];
        int to = 0;
        for (int j = 1; j < fits; ++j) if (fill[j] <= fill[to]) to = j;
        const int slot = fill[to]++ * bestp + to;
        if (slot >= kFusedTileTracks * tps) return;   // (rows_of said it fits: not reached; equal slices stay)
        slot_of[i] = slot; sc_slots[sc] = std::max(sc_slots[sc], slot + 1);
      }
      dealt_rows += *std::max_element(fill, fill + bestp);
    }
    // rows_of() is the closed form of what this dealing reaches (most demanding first, emptiest fitting slice: optimal for nested
    // slices); the shape was chosen on it, so a dealing that needs more rows does not stand
    if (dealt_rows != best_rows) { shape_mismatches().fetch_add(1, std::memory_order_relaxed); return; }
    for (int i = 0; i < ntrk; ++i)
      for (int s = run_trk[i].s0; s < run_trk[i].s0 + run_trk[i].len; ++s) obs_tl[s] = (uint8_t)slot_of[i];
    for (int sc = 0; sc < nsc; ++sc) fp.tile_trk_end[(size_t)run_tile0 + std::min(run_ntiles, (sc + 1) * tps) - 1] = sc_slots[sc];
    r.gp = 1 | (bestp << 8) | kFusedUnequalSlices;
    for (int j = 0, at = 0; j < bestp; ++j) { fp.tgts.push_back((unsigned short)(at | (best[j] << 8))); at += best[j]; }
  };
  auto finalize_run = [&]() {
    if (!run_ntiles) { run_cams.clear(); run_pairs.clear(); run_ccams.clear(); run_trk.clear(); run_kmin = 64; run_obs = 0; run_key0 = -1; ++serial; return; }
    std::sort(run_cams.begin(), run_cams.end());
    std::sort(run_pairs.begin(), run_pairs.end());
    FusedRun r;
    r.tile0 = run_tile0; r.ntiles = run_ntiles;
    r.cam_off = (int)fp.cams.size(); r.W = (int)run_cams.size();
    fp.cams.insert(fp.cams.end(), run_cams.begin(), run_cams.end());
    r.tgt_off = (int)fp.tgts.size(); r.ntgt = (int)run_pairs.size();
    for (size_t i = 0; i < run_cams.size(); ++i) cam_local[run_cams[i]] = (uint8_t)i;   // local index by table, not by search
    for (int64_t key : run_pairs) {   // ascending (hi, lo) -> ascending (la, lb)
      const int la = cam_local[(int)(key >> 32)], lb = cam_local[(int)(key & 0xffffffff)];
      fp.tgts.push_back((unsigned short)(la | (lb << 8)));
    }
    const int need = (int)std::max(lanes_tgt * r.ntgt, rows_cam * r.W);
    const int G = need <= 64 ? 1 : (need <= 128 ? 2 : 4);
    r.gp = G | ((G == 1 ? std::max(1, packing((size_t)r.ntgt, (size_t)r.W)) : 1) << 8);
    if (bw == 0 && G == 1 && unequal_slices) shape_slices(r);
    r.part_off = (int)fp.part_doubles;
    fp.part_doubles += (size_t)r.ntgt * part_tgt + (size_t)r.W * part_cam;
    r.stage_off = (int)fp.stage.size();
    for (int pc : run_cams) fp.stage.push_back(h->part_cam[pc]);
    fp.stage.insert(fp.stage.end(), run_ccams.begin(), run_ccams.end());
    r.nstage = (int)(run_cams.size() + run_ccams.size());
    for (int t = run_tile0; t < run_tile0 + run_ntiles; ++t)
      for (int s = tstart[t]; s < tstart[t] + tcount[t]; ++s) {
        if (sred[s] >= 0) obs_lc[s] = cam_local[sred[s]];
        else obs_lc[s] = (uint8_t)(0x80 | ccam_local[ocam[s]]);
      }
    fp.runs.push_back(r);
    run_tile0 += run_ntiles; run_ntiles = 0; run_obs = 0; run_key0 = -1;
    run_cams.clear(); run_pairs.clear(); run_ccams.clear(); run_trk.clear(); run_kmin = 64; ++serial;
  };
  auto push_long = [&](int q) {
    const int slot = (int)l_pt.size();
    l_pt.push_back(porder[q]);
    for (int64_t c = off[q]; c < off[q + 1]; ++c) { l_obs.push_back((int)c); l_slot.push_back(slot); }
    l_start.push_back((int)l_obs.size());
  };
  run_tile0 = (int)tstart.size();
  for (int q = q_begin; q < q_end; ++q) {
    const int64_t L = off[q + 1] - off[q];
    if (L == 0) continue;
    // the track's variable cameras
    tc.clear(); tcc.clear();
    for (int64_t s = off[q]; s < off[q + 1]; ++s) {
      if (sred[s] >= 0) tc.push_back(sred[s]);
      else tcc.push_back(ocam[s]);
    }
    std::sort(tc.begin(), tc.end());
    const bool dup = std::adjacent_find(tc.begin(), tc.end()) != tc.end();
    if (!tcc.empty()) { std::sort(tcc.begin(), tcc.end()); tcc.erase(std::unique(tcc.begin(), tcc.end()), tcc.end()); }
    mark_tiles(q);
    if (L > 64 || dup || (int)tc.size() > max_cams || (int)tcc.size() > max_const) {
      close_tile(q);            // tiles are contiguous observation ranges
      push_long(q);
      continue;
    }
    // a camera set that already joined this run (tracks are ordered by first camera: common): nothing new
    unsigned set_hash = (unsigned)tc.size();
    for (int c : tc) set_hash = set_hash * 0x9E3779B1u + (unsigned)c;
    SeenSet& seen = seen_sets[(set_hash >> 16) & (kSeenSets - 1)];
    const int prev_serial = serial;   // (the run open when the set was looked up)
    const bool same_set = seen.stamp == serial && seen.n == (int)tc.size() && std::equal(tc.begin(), tc.end(), seen.cams);
    size_t ucams = run_cams.size(), upairs = run_pairs.size();
    if (!same_set) {
      tp.clear();
      for (size_t a = 0; a < tc.size(); ++a)
        for (size_t b = 0; b <= a; ++b) tp.push_back(((int64_t)tc[a] << 32) | (uint32_t)tc[b]);
      // would the run still fit?  sizes of the unions with the run's sets
      for (int c : tc) ucams += cam_stamp[c] != serial;
      for (int64_t key : tp) upairs += pair_stamp[pair_slot(key)] != serial;
    }
    bool new_run = (int)ucams > max_cams || upairs > max_tgts;
    if (!tcc.empty()) {
      size_t uc = run_ccams.size();
      for (int c : tcc) uc += ccam_stamp[c] != serial;
      if (uc > (size_t)max_const) new_run = true;
    }
    // a run keeps its packing level (track slices per wave) once it has some work, and stays inside one
    // first-camera key once it is large enough
    // (compound blocks: the level is the number of track slices a workgroup walks in parallel -- 4 / G, or 4 PS with one
    // wave per slice -- so that a run of short tracks, two slices, does not absorb the long tracks of the same cameras)
    auto level = [&](size_t ntgt, size_t W) -> int {
      const int pk = packing(ntgt, W);
      if (bw == 0 || pk > 0) return bw == 0 ? pk : 4;   // (one wave per slice: four slices or more, all the same to this rule)
      const size_t need = std::max(lanes_tgt * ntgt, rows_cam * W);
      return need <= 128 ? 2 : 1;
    };
    if (!new_run && run_obs >= 64 && level(upairs, ucams) < level(run_pairs.size(), run_cams.size())) new_run = true;
    if (!new_run && run_obs >= run_max / 4 && skey[q] != run_key0) new_run = true;
    if (new_run) {
      close_tile(q);
      finalize_run();
    }
    if (t_len + L > 64 || t_tracks >= kFusedTileTracks) {
      close_tile(q);
      // runs that need several waves per track slice walk their tracks (almost) serially: keep them short, so that
      // many workgroups share that work instead of a few long ones setting the kernel's duration
      const size_t need = std::max(lanes_tgt * run_pairs.size(), rows_cam * run_cams.size());
      // (compound blocks: nearly every run needs the whole workgroup per track slice, and a run's partial blocks are 44 KB --
      // one run per sub-chunk wrote 420 MB of them per iteration at 1000 views / 500k tracks)
      const int64_t cap = bw ? run_max : (need <= 64 ? run_max : (need <= 128 ? run_max / 4 : 1));
      if (run_ntiles % tps == 0 && run_obs >= cap) finalize_run();
    }
    if (t_len == 0) {
      t_start = off[q];
      if (run_ntiles % tps == 0) sc_tracks = 0;
      if (run_key0 < 0) run_key0 = skey[q];
    }
    for (int64_t s = off[q]; s < off[q + 1]; ++s) obs_tl[s] = (uint8_t)sc_tracks;
    sc_tracks++; t_tracks++; t_len += L; run_obs += L;
    // the track joins the open run
    if (!(same_set && serial == prev_serial)) {   // (a run closed above: the sets are empty again and tp may be stale)
      if (same_set) {
        tp.clear();
        for (size_t a = 0; a < tc.size(); ++a)
          for (size_t b = 0; b <= a; ++b) tp.push_back(((int64_t)tc[a] << 32) | (uint32_t)tc[b]);
      }
      for (int c : tc) if (cam_stamp[c] != serial) { cam_stamp[c] = serial; run_cams.push_back(c); }
      for (int64_t key : tp) {
        const int sl = pair_slot(key);
        if (pair_stamp[sl] != serial) { pair_stamp[sl] = serial; pair_key[sl] = key; run_pairs.push_back(key); }
      }
      seen.stamp = serial; seen.n = (int)tc.size();
      std::copy(tc.begin(), tc.end(), seen.cams);
    }
    for (int c : tcc) if (ccam_stamp[c] != serial) { ccam_stamp[c] = serial; ccam_local[c] = (uint8_t)run_ccams.size(); run_ccams.push_back(c); }
    run_trk.push_back(RunTrack{(int)off[q], tc.empty() ? -1 : tc.back(), (int)tstart.size(), (uint8_t)L, 0});
    run_kmin = std::min(run_kmin, (int)tc.size());
  }
  close_tile(q_end);
  finalize_run();
}

// Sum lists of the fused assembly with intrinsics (k_sum_items, ba_fused_intr.hip): per block of S (camera x camera,
// camera x group, group x group) and per vector block (rhs / gradient / column norms of a camera or a group) the pieces of
// the runs' partial blocks that feed it, in run order.  A run's target (la, lb) holds the compound block
// [cam_a | intr_a] x [cam_b | intr_b] as if the two cameras owned their intrinsics; the intrinsics rows / columns of every
// camera of a group land on the group's (bundle_adjuster.cc:463-475: the cameras of a group share ONE parameter block).
// Lists longer than 2 x chunk go through intermediate sums (SK_CHUNK items) and a second-level item.
int build_sum_items_intr(theia_ba_handle_s* h, const int* cam_group, FusedHost& fp, int* n_items1, int* n_items2) {
  constexpr int SK_BLOCK = 0, SK_LOWER = 1, SK_VEC = 2, SK_CHUNK = 3;
  const int KI = h->fused_bw - 6, ni = h->ni, BW = h->fused_bw;   // a run's partial blocks: BW x BW per target (row stride BW), BW x 3 per camera
  struct Ent { int64_t key; int off, code, dims; };   // dims = nr | nc << 4 | kind << 8 | rgrp << 12 | cgrp << 13
  auto src_code = [](int r0, int c0, int tr, int stride) { return r0 | (c0 << 4) | (tr << 8) | (stride << 16); };
  auto dims = [](int nr, int nc, int kind, int rg, int cg) { return nr | (nc << 4) | (kind << 8) | (rg << 12) | (cg << 13); };
  auto key_blk = [](int row0, int col0) { return ((int64_t)row0 << 30) | (int64_t)col0; };
  auto key_vec = [](int row0) { return ((int64_t)1 << 60) | ((int64_t)row0 << 30); };
  // The entries of fixed ranges of runs on host threads, in run order: one pass counts, one writes.  They live in blocks of
  // the pinned host cache -- three fresh 18 MB vectors cost more in page faults than the sort that fills them.
  constexpr int kRunParts = 32;
  const int nruns = (int)fp.runs.size();
  auto emit = [&](int ir, auto&& sink) {
    const FusedRun& r = fp.runs[ir];
    auto cam_of = [&](int l) { return h->part_cam[fp.cams[r.cam_off + l]]; };
    for (int k = 0; k < r.ntgt; ++k) {
      const unsigned us = fp.tgts[r.tgt_off + k];
      const int la = us & 0xff, lb = us >> 8;
      const int ca = cam_of(la), cb = cam_of(lb);
      const int rca = h->cam_red[ca], rcb = h->cam_red[cb], ga = h->grp_red[cam_group[ca]], gb = h->grp_red[cam_group[cb]];
      const int base = r.part_off + BW * BW * k;
      if (rca >= 0 && rcb >= 0)
        sink(Ent{key_blk(ni + 6 * rca, ni + 6 * rcb), base, src_code(0, 0, 0, BW), dims(6, 6, la == lb ? SK_LOWER : SK_BLOCK, 0, 0)});
      if (rca >= 0 && gb >= 0)
        sink(Ent{key_blk(ni + 6 * rca, 10 * gb), base, src_code(0, 6, 0, BW), dims(6, KI, SK_BLOCK, 0, 1)});
      if (la != lb && rcb >= 0 && ga >= 0)
        sink(Ent{key_blk(ni + 6 * rcb, 10 * ga), base, src_code(6, 0, 1, BW), dims(6, KI, SK_BLOCK, 0, 1)});
      if (ga >= 0 && gb >= 0) {
        // (an item is one wave: nr x nc <= 64 elements.  Up to seven compact rows a group x group block is one item; the 10 x 10
        // blocks of the 16-row plan go as two items of five compact rows, item row0 = 10 g + first compact row)
        const int nh = KI > 7 ? 2 : 1, hr = KI > 7 ? KI / 2 : KI;
        for (int hh = 0; hh < nh; ++hh) {
          const int r0 = hh * hr, nr = (hh == nh - 1) ? KI - r0 : hr;
          if (ga > gb) sink(Ent{key_blk(10 * ga + r0, 10 * gb), base, src_code(6 + r0, 6, 0, BW), dims(nr, KI, SK_BLOCK, 1, 1)});
          else if (ga < gb) sink(Ent{key_blk(10 * gb + r0, 10 * ga), base, src_code(6, 6 + r0, 1, BW), dims(nr, KI, SK_BLOCK, 1, 1)});
          else {
            sink(Ent{key_blk(10 * ga + r0, 10 * ga), base, src_code(6 + r0, 6, 0, BW), dims(nr, KI, SK_LOWER, 1, 1)});
            if (la != lb) sink(Ent{key_blk(10 * ga + r0, 10 * ga), base, src_code(6, 6 + r0, 1, BW), dims(nr, KI, SK_LOWER, 1, 1)});
          }
        }
      }
    }
    for (int l = 0; l < r.W; ++l) {
      const int c = cam_of(l), rc = h->cam_red[c], gr = h->grp_red[cam_group[c]];
      const int base = r.part_off + BW * BW * r.ntgt + 3 * BW * l;
      if (rc >= 0) sink(Ent{key_vec(ni + 6 * rc), base, src_code(0, 0, 0, 3), dims(6, 3, SK_VEC, 0, 0)});
      if (gr >= 0) sink(Ent{key_vec(10 * gr), base, src_code(6, 0, 0, 3), dims(KI, 3, SK_VEC, 1, 0)});
    }
  };
  std::vector<size_t> at(kRunParts + 1, 0);
  host_parts(kRunParts, nruns >= 256, [&](int part) {
    size_t cnt = 0;
    for (int ir = (int)((int64_t)nruns * part / kRunParts); ir < (int)((int64_t)nruns * (part + 1) / kRunParts); ++ir) emit(ir, [&](const Ent&) { ++cnt; });
    at[part + 1] = cnt;
  });
  for (int k = 0; k < kRunParts; ++k) at[k + 1] += at[k];
  const size_t nent = at[kRunParts];
  HBuf<Ent> ents_b, tmp_b;
  if (!ents_b.resize(std::max<size_t>(1, nent), true) || !tmp_b.resize(std::max<size_t>(1, nent), true)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %zu sum-list entries failed", nent);
  Ent* const ents = ents_b.data();
  host_parts(kRunParts, nruns >= 256, [&](int part) {
    Ent* out = ents + at[part];
    for (int ir = (int)((int64_t)nruns * part / kRunParts); ir < (int)((int64_t)nruns * (part + 1) / kRunParts); ++ir) emit(ir, [&](const Ent& e) { *out++ = e; });
  });
  {   // ascending key = (vector blocks last, row, column), ties in run order: two stable counting passes over the row / column
      // offsets (a std::stable_sort of the 0.8 M entries of the 1000-view configuration took 30 ms of the create())
    const int nb = h->n + 2;
    counting_pass(ents, tmp_b.data(), (int64_t)nent, nb, [](const Ent& e) { return (int)(e.key & 0x3fffffff); });
    counting_pass(tmp_b.data(), ents, (int64_t)nent, 2 * nb, [nb](const Ent& e) { return (int)((e.key >> 30) & 0x3fffffff) + ((e.key >> 60) ? nb : 0); });
  }
  std::vector<int> items1, items2, src2;
  fp.sum_src.clear();
  fp.sum_src.reserve(2 * nent);
  for (size_t k = 0; k < nent; ++k) { fp.sum_src.push_back(ents[k].off); fp.sum_src.push_back(ents[k].code); }
  size_t chunk_off = fp.part_doubles;
  auto push = [](std::vector<int>& v, int row0, int col0, int code, int beg, int end, int dst) {
    v.push_back(row0); v.push_back(col0); v.push_back(code); v.push_back(beg); v.push_back(end); v.push_back(dst);
  };
  const int nsrc1 = (int)nent;
  for (size_t q = 0; q < nent;) {
    size_t e = q;
    while (e < nent && ents[e].key == ents[q].key) ++e;
    const int row0 = (int)((ents[q].key >> 30) & 0x3fffffff), col0 = (int)(ents[q].key & 0x3fffffff);
    const int code = ents[q].dims, nr = code & 15, nc = (code >> 4) & 15;
    const size_t cnt = e - q;
    size_t ch = 96;   // sources per first-level chunk: a wave adds them with 64 / (nr nc) lane groups, eight loads in flight each
    while (ch * ch < cnt) ++ch;
    if (cnt <= 2 * ch) {
      push(items1, row0, col0, code, (int)q, (int)e, 0);
    } else {
      const int beg2 = nsrc1 + (int)src2.size() / 2;
      for (size_t c0 = q; c0 < e; c0 += ch) {
        push(items1, 0, 0, (code & 0xff) | (SK_CHUNK << 8), (int)c0, (int)std::min(e, c0 + ch), (int)chunk_off);
        src2.push_back((int)chunk_off); src2.push_back(nc << 16);
        chunk_off += (size_t)nr * nc;
      }
      push(items2, row0, col0, code, beg2, nsrc1 + (int)src2.size() / 2, 0);
    }
    q = e;
  }
  fp.sum_src.insert(fp.sum_src.end(), src2.begin(), src2.end());
  if (getenv("THEIA_HIP_CREATE_TIMING")) {
    size_t longest = 0, nchunk = 0;
    for (size_t k = 0; k < items1.size(); k += 6) {
      longest = std::max<size_t>(longest, (size_t)(items1[k + 4] - items1[k + 3]));
      nchunk += ((items1[k + 2] >> 8) & 15) == SK_CHUNK;
    }
    fprintf(stderr, "theia_hip sum lists: %zu first-level items (%zu chunks), %zu second-level, %d + %zu sources, longest list %zu, "
            "%zu partial doubles + %zu chunk doubles\n", items1.size() / 6, nchunk, items2.size() / 6, nsrc1, src2.size() / 2, longest,
            fp.part_doubles, chunk_off - fp.part_doubles);
  }
  fp.part_doubles = chunk_off;
  *n_items1 = (int)items1.size() / 6; *n_items2 = (int)items2.size() / 6;
  fp.sum_items = items1;
  fp.sum_items.insert(fp.sum_items.end(), items2.begin(), items2.end());
  return 0;
}

// The segments in order -> one plan (offsets rebased), then per S block the partial sums that feed it, in run order.
void merge_fused_segments(const theia_ba_handle_s* h, std::vector<FusedSegment>& segs, std::vector<int>& tstart, std::vector<int>& tcount,
                          std::vector<int>& tkey, std::vector<int>& l_obs, std::vector<int>& l_slot, std::vector<int>& l_start,
                          std::vector<int>& l_pt, FusedHost& fp) {
  const int adj_nt = (h->n + 63) / 64;
  fp.tile_adj.assign((size_t)adj_nt * adj_nt, 0);
  for (FusedSegment& sg : segs) {
    const int tile0 = (int)tstart.size(), cam0 = (int)fp.cams.size(), tgt0 = (int)fp.tgts.size(), stage0 = (int)fp.stage.size();
    const int slot0 = (int)l_pt.size(), lobs0 = (int)l_obs.size();
    tstart.insert(tstart.end(), sg.tstart.begin(), sg.tstart.end());
    tcount.insert(tcount.end(), sg.tcount.begin(), sg.tcount.end());
    tkey.insert(tkey.end(), sg.tkey.begin(), sg.tkey.end());
    for (FusedRun r : sg.fp.runs) {
      r.tile0 += tile0; r.cam_off += cam0; r.tgt_off += tgt0; r.part_off += (int)fp.part_doubles; r.stage_off += stage0;
      fp.runs.push_back(r);
    }
    fp.part_doubles += sg.fp.part_doubles;
    fp.cams.insert(fp.cams.end(), sg.fp.cams.begin(), sg.fp.cams.end());
    fp.stage.insert(fp.stage.end(), sg.fp.stage.begin(), sg.fp.stage.end());
    fp.tgts.insert(fp.tgts.end(), sg.fp.tgts.begin(), sg.fp.tgts.end());
    fp.tile_trk_end.insert(fp.tile_trk_end.end(), sg.fp.tile_trk_end.begin(), sg.fp.tile_trk_end.end());
    l_obs.insert(l_obs.end(), sg.l_obs.begin(), sg.l_obs.end());
    for (int v : sg.l_slot) l_slot.push_back(v + slot0);
    for (int v : sg.l_start) l_start.push_back(v + lobs0);
    l_pt.insert(l_pt.end(), sg.l_pt.begin(), sg.l_pt.end());
    for (size_t i = 0; i < fp.tile_adj.size(); ++i) fp.tile_adj[i] |= sg.fp.tile_adj[i];
  }
  const bool ptiming = getenv("THEIA_HIP_CREATE_TIMING") != nullptr;
  auto pt0 = std::chrono::steady_clock::now();
  auto ptick = [&](const char* what) {
    if (!ptiming) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "theia_hip create:     fused plan: %-18s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - pt0).count());
    pt0 = t;
  };
  ptick("(since runs built)");
  if (h->fused_bw) return;   // compound blocks: build_sum_items_intr (create())
  // per S block: the partial sums that feed it, in run order
  struct Ent { int64_t key; int src; int isd; };
  std::vector<Ent> ents;
  for (const FusedRun& r : fp.runs) {
    for (int k = 0; k < r.ntgt; ++k) {
      const unsigned us = fp.tgts[r.tgt_off + k];
      const int ri = fp.cams[r.cam_off + (us & 0xff)], rj = fp.cams[r.cam_off + (us >> 8)];
      ents.push_back({((int64_t)ri << 32) | (uint32_t)rj, r.part_off + 36 * k, 0});
    }
    for (int lc = 0; lc < r.W; ++lc) {
      const int ri = fp.cams[r.cam_off + lc];
      ents.push_back({((int64_t)ri << 32) | (uint32_t)ri, r.part_off + 36 * r.ntgt + 18 * lc, 1});
    }
  }
  {   // order (row camera, column camera, block pieces before diagonal pieces, run order): three stable counting passes, least
      // significant key first (std::stable_sort on the 230 k entries of the 1000-view configuration took 2.3 ms of the create())
    const int nb = std::max(2, h->ncp) + 1;
    std::vector<Ent> tmp(ents.size());
    const int64_t ne = (int64_t)ents.size();
    counting_pass(ents.data(), tmp.data(), ne, nb, [](const Ent& en) { return en.isd; });
    counting_pass(tmp.data(), ents.data(), ne, nb, [](const Ent& en) { return (int)(en.key & 0xffffffff); });
    counting_pass(ents.data(), tmp.data(), ne, nb, [](const Ent& en) { return (int)(en.key >> 32); });
    ents.swap(tmp);
  }
  for (size_t q = 0; q < ents.size();) {
    size_t e = q;
    while (e < ents.size() && ents[e].key == ents[q].key) ++e;
    size_t m = q;
    while (m < e && !ents[m].isd) ++m;
    fp.sum_items.push_back((int)(ents[q].key >> 32)); fp.sum_items.push_back((int)(ents[q].key & 0xffffffff));
    fp.sum_items.push_back((int)q); fp.sum_items.push_back((int)m);
    fp.sum_items.push_back((int)m); fp.sum_items.push_back((int)e);
    q = e;
  }
  fp.sum_src.reserve(ents.size());
  for (const Ent& en : ents) fp.sum_src.push_back(en.src);
  ptick("sum items");
}

#undef UP
#undef AL
// (private return code of ba_create_impl: the fused intrinsics plan does not fit this problem, build it again on the gather lists)
constexpr int kRetryWithoutFusedIntr = 0x7a11;
// Problem structure (bundle_adjuster.cc:116-221,357-380,477-527): the variable cameras and intrinsics groups, their reduced indices
// and masks, the reduced system's size, the cameras of the fused Schur assembly.  Reads p, o and the used flags; no device memory.
void classify_blocks(theia_ba_handle_s* h, const theia_ba_problem* p, const theia_ba_options* o, const std::vector<uint8_t>& cam_used,
                     const std::vector<uint8_t>& grp_used, bool allow_fused_intr) {
  h->cam_red.assign(h->nc, -1); h->cam_mask.assign(h->nc, 0x3f); h->pt_const.assign(h->np, 1);
  h->ncv = 0;
  for (int c = 0; c < h->nc; ++c) {
    unsigned m = p->cam_const ? p->cam_const[c] : 0;
    if (o->constant_camera_orientation) m |= THEIA_CAM_CONST_ORIENTATION;
    if (o->constant_camera_position) m |= THEIA_CAM_CONST_POSITION;
    if (o->orthographic_camera) m |= THEIA_CAM_CONST_TZ;
    unsigned cols = 0;
    if (m & THEIA_CAM_CONST_POSITION) cols |= 0x07;
    if (m & THEIA_CAM_CONST_ORIENTATION) cols |= 0x38;
    if (m & THEIA_CAM_CONST_TZ) cols |= 0x04;
    if (cols != 0x3f && (cam_used[c] || (p->flags & THEIA_BA_FLAG_KEEP_UNOBSERVED_CAMERAS))) { h->cam_red[c] = h->ncv++; h->cam_mask[c] = (uint8_t)cols; }
  }
  // intrinsics blocks (bundle_adjuster.cc:382-460): constant when nothing is optimised
  // or the caller marked the group constant, otherwise a subset manifold
  h->grp_red.assign(h->ng, -1); h->grp_free.assign(h->ng, 0u); h->grp_k.assign(h->ng, 0);
  h->ngv = 0;
  for (int g = 0; g < h->ng; ++g) {
    h->grp_k[g] = intrinsics_size(p->group_model[g]);
    const unsigned fm = intrinsics_free_mask(p->group_model[g], o->intrinsics_to_optimize);
    const bool gconst = (p->group_const && p->group_const[g]) || fm == 0 ||
                        (!grp_used[g] && !(p->flags & THEIA_BA_FLAG_KEEP_UNOBSERVED_CAMERAS));
    if (!gconst) { h->grp_red[g] = h->ngv++; h->grp_free[g] = fm; }
  }
  h->ni = THEIA_MAX_INTRINSICS * h->ngv;
  h->n = h->ni + 6 * h->ncv;
  {   // fused assembly with intrinsics (ba_fused_intr.hip): compact rows, at most four free parameters per group
    int most = 0;
    for (int g = 0; g < h->ng; ++g) if (h->grp_red[g] >= 0) most = std::max(most, __builtin_popcount(h->grp_free[g]));
    const char* force = getenv("THEIA_HIP_INTR_ROWS");
    // (block width 6 + rows: 9, 10, 13 for five to seven free parameters -- every intrinsic of the pinhole model --, 16 for up to
    // the ten of the radial-tangential model)
    h->fused_bw = (allow_fused_intr && h->ni > 0 && !(force && atoi(force) == 10) && !getenv("THEIA_HIP_INTR_GATHER")) ? (most <= 3 ? 9 : (most <= 4 ? 10 : (most <= 7 ? 13 : 16))) : 0;
    h->fused_kmask = 0;
    {
      bool first = true, same = true;
      for (int g = 0; g < h->ng; ++g) if (h->grp_red[g] >= 0) { if (first) { h->fused_kmask = h->grp_free[g]; first = false; } else if (h->grp_free[g] != h->fused_kmask) same = false; }
      if (!same) h->fused_kmask = 0;
    }
    h->cam_part.assign(h->nc, -1);
    h->ncp = 0;
    for (int c = 0; c < h->nc; ++c)
      if (h->cam_red[c] >= 0 || (h->fused_bw && cam_used[c] && h->grp_red[p->cam_group[c]] >= 0)) { h->cam_part[c] = h->ncp++; h->part_cam.push_back(c); }
  }
}

int ba_create_impl(const theia_ba_problem* p, const theia_ba_options* o, theia_ba_handle* out, bool allow_fused_intr) {
  if (!out) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "null handle pointer");
  *out = nullptr;
  int rc = validate(p, o);
  if (rc) return rc;
  if (p->flags & THEIA_BA_FLAG_INVERSE_DEPTH) {
    std::unique_ptr<theia_ba_handle_s> hi(new theia_ba_handle_s());
    hi->opt = *o;
    hi->nc = p->num_cameras; hi->ng = p->num_groups; hi->np = p->num_points; hi->nobs = p->num_obs;
    if ((rc = thip::id_handle_create(p, o, &hi->idh))) return rc;
    *out = hi.release();
    return 0;
  }
  rc = thip::ensure_device();
  if (rc) return rc;
  theia_ba_handle_s* h = new theia_ba_handle_s();
  std::unique_ptr<theia_ba_handle_s> guard(h);
  h->opt = *o;
  h->nc = p->num_cameras; h->ng = p->num_groups; h->np = p->num_points; h->nobs = p->num_obs;
  h->pd = o->use_homogeneous_point_parametrization ? 3 : 4;
  HIP_TRYR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->stage.stream = h->stream;
  StageScope stage_scope(&h->stage);
  PoolStreamScope pool_scope(h->stream);   // blocks that go back to the caches inside this call are tagged with an event on it
  for (auto& row : h->ev) for (auto& e : row) HIP_TRYR(hipEventCreate(&e));
  HIP_TRYR(hipHostMalloc((void**)&h->h_scal, sizeof(double) * 40, hipHostMallocDefault));
  HIP_TRYR(hipHostMalloc((void**)&h->h_state, kLmBlockBytes, hipHostMallocDefault));

  // THEIA_HIP_CREATE_TIMING=1: wall time of the create() stages on stderr
  const bool ctiming = getenv("THEIA_HIP_CREATE_TIMING") != nullptr;
  auto ct0 = std::chrono::steady_clock::now();
  auto tick = [&](const char* what) {
    if (!ctiming) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "theia_hip create: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - ct0).count());
    ct0 = t;
  };
  tick("stream + events");
  // --- problem structure (bundle_adjuster.cc:116-221,357-380,477-527) ---
  std::vector<uint8_t> cam_used(h->nc, 0);
  RawArray<uint8_t> pt_used((size_t)h->np);
  std::vector<uint8_t> grp_used(h->ng, 0);
  std::vector<int> toff((size_t)h->np + 1, 0);   // the track CSR (below)
  std::atomic<int> unsorted{0};
  {   // cameras with observations: flags per host thread, merged (the tracks' flags come with the key pass below)
    std::mutex mu;
    host_chunks(h->nobs, [&](int64_t i0, int64_t i1) {
      std::vector<uint8_t> mine(h->nc, 0);
      bool disorder = false;   // (the same pass: does the input come track by track?  see the track CSR below)
      for (int64_t i = i0; i < i1; ++i) {
        mine[p->obs_cam[i]] = 1;
        const int q1 = p->obs_pt[i], q0 = i ? p->obs_pt[i - 1] : -1;
        disorder |= q1 < q0;
        for (int q = q0 + 1; q <= q1; ++q) toff[q] = (int)i;   // toff[q] = first observation of a track >= q (meaningful if no disorder)
      }
      if (disorder) unsorted.store(1, std::memory_order_relaxed);
      std::lock_guard<std::mutex> lk(mu);
      for (int c = 0; c < h->nc; ++c) cam_used[c] |= mine[c];
    });
    for (int c = 0; c < h->nc; ++c) if (cam_used[c]) grp_used[p->cam_group[c]] = 1;
  }
  classify_blocks(h, p, o, cam_used, grp_used, allow_fused_intr);

  // Tracks are visited in the order of their first (lowest) variable camera of
  // the reduced ordering, so that a workgroup's tile range touches a short
  // window of cameras (LDS accumulation in k_linearize).  Observations are
  // sorted by that track order; residual blocks whose blocks are all constant
  // are evaluated once ("fixed cost", ceres reduced program).
  RawArray<uint8_t> fixed((size_t)h->nobs);   // (these four are written by the per-track pass below)
  RawArray<int> pkey((size_t)h->np);
  RawArray<int> nvar((size_t)h->np);   // variable cameras of a track
  // The input's observations grouped by track (CSR): toff[q] .. toff[q + 1] are track q's entries of tobs, in input order.
  // Input that already comes track by track (obs_pt non-decreasing: what a flattened reconstruction looks like) needs no
  // index array; anything else is counted, scattered with atomic cursors and put back into input order per track.
  HBuf<int> tobs_b;
  const int* tobs = nullptr;   // nullptr: the identity
  {
    if (!unsorted.load()) {   // (the offsets were written by the first pass over the observations, above)
      for (int q = h->nobs ? p->obs_pt[h->nobs - 1] + 1 : 0; q <= h->np; ++q) toff[q] = (int)h->nobs;
    } else {
      std::fill(toff.begin(), toff.end(), 0);
      if (!tobs_b.resize((size_t)std::max<int64_t>(1, h->nobs), true)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %lld observations failed", (long long)h->nobs);
      int* const tb = tobs_b.data();
      host_chunks(h->nobs, [&](int64_t i0, int64_t i1) { for (int64_t i = i0; i < i1; ++i) __atomic_fetch_add(&toff[(size_t)p->obs_pt[i] + 1], 1, __ATOMIC_RELAXED); });
      for (int q = 0; q < h->np; ++q) toff[q + 1] += toff[q];
      std::vector<int> cur(toff.begin(), toff.end() - 1);
      host_chunks(h->nobs, [&](int64_t i0, int64_t i1) { for (int64_t i = i0; i < i1; ++i) tb[__atomic_fetch_add(&cur[p->obs_pt[i]], 1, __ATOMIC_RELAXED)] = (int)i; });
      host_chunks(h->np, [&](int64_t q0, int64_t q1) { for (int64_t q = q0; q < q1; ++q) std::sort(tb + toff[q], tb + toff[q + 1]); });
      tobs = tb;
    }
  }
  RawArray<int> nfix((size_t)h->np);   // residual blocks of a track whose blocks are all constant
  host_chunks(h->np, [&](int64_t q0, int64_t q1) {   // per-track sums: tracks are independent
    for (int64_t q = q0; q < q1; ++q) {
      pt_used[q] = toff[q + 1] > toff[q];
      const bool qconst = p->point_const && p->point_const[q];
      int nv = 0, pk = std::numeric_limits<int>::max(), nf = 0;
      for (int k = toff[q]; k < toff[q + 1]; ++k) {
        const int i = tobs ? tobs[k] : k;
        const int c = p->obs_cam[i];
        const int rc = h->cam_part[c];
        if (rc >= 0) { nv++; if (rc < pk) pk = rc; }
        // a residual block whose blocks are all constant (an observed track is constant iff the caller marked it)
        fixed[i] = (qconst && h->cam_red[c] < 0 && h->grp_red[p->cam_group[c]] < 0) ? 1 : 0;
        nf += fixed[i];
      }
      nvar[q] = nv; pkey[q] = pk; nfix[q] = nf;
      h->pt_const[q] = ((p->point_const && p->point_const[q]) || !pt_used[q]) ? 1 : 0;
    }
  });
  std::vector<int> porder(h->np);
  // Inside one first-camera key, short tracks come first (classes by number of variable cameras): the fused Schur
  // kernel packs several short tracks into one wave step when a run of tracks touches few target blocks.
  RawArray<int> skey_pt((size_t)h->np);
  std::atomic<int> maxkey_all{-1};
  host_chunks(h->np, [&](int64_t q0, int64_t q1) {
    int mk = -1;
    for (int64_t q = q0; q < q1; ++q) {
      porder[q] = (int)q;
      // measured at 1k views / 500k tracks (K1 + K2 launch group): {<= 7 | >= 8} 0.575 ms, {<= 6 | >= 7} 0.599, {<= 5 | >= 6} 0.670,
      // {<= 8 | >= 9} 0.646, {<= 3 | 4..6 | >= 7} 0.636, one class 0.593
      static const int ncls = getenv("THEIA_HIP_FUSED_CLASSES") ? atoi(getenv("THEIA_HIP_FUSED_CLASSES")) : 2;
      static const int cut0 = getenv("THEIA_HIP_FUSED_CUT0") ? atoi(getenv("THEIA_HIP_FUSED_CUT0")) : 7;
      int cls = ncls == 2 ? (nvar[q] <= cut0 ? 0 : 2) : (nvar[q] <= 3 ? 0 : (nvar[q] <= 6 ? 1 : 2));
      {   // development: THEIA_HIP_FUSED_CUTS="a,b,c" -> classes {<= a | <= b | <= c | more}
        static const std::vector<int> cuts = [] { std::vector<int> v; const char* e = getenv("THEIA_HIP_FUSED_CUTS"); if (e) { for (const char* c = e; *c;) { v.push_back(atoi(c)); while (*c && *c != ',') ++c; if (*c) ++c; } } return v; }();
        if (!cuts.empty()) { cls = 0; for (int cu : cuts) if (nvar[q] > cu) ++cls; cls = std::min(cls, 3); }
      }
      // compound blocks (three or four lanes per target): four classes, by the number of track slices a workgroup can walk
      // in parallel -- <= 3 cameras and 4 .. 6: four slices; 7: two; more: one
      if (h->fused_bw && !getenv("THEIA_HIP_FUSED_CLASSES")) cls = nvar[q] <= 3 ? 0 : (nvar[q] <= 6 ? 1 : (nvar[q] <= 7 ? 2 : 3));
      static const bool noclass = getenv("THEIA_HIP_FUSED_NOCLASS") != nullptr;
      skey_pt[q] = pkey[q] == std::numeric_limits<int>::max() ? pkey[q] : (((h->ni == 0 || h->fused_bw) && !noclass) ? pkey[q] * 4 + cls : pkey[q]);
      if (skey_pt[q] != std::numeric_limits<int>::max()) mk = std::max(mk, skey_pt[q]);
    }
    int cur = maxkey_all.load();
    while (mk > cur && !maxkey_all.compare_exchange_weak(cur, mk)) {}
  });
  tick("  structure: masks, keys");
  // Stable counting sort of the tracks by key (keys are < 4 * (#variable cameras) + 4, or INT_MAX = no variable camera: last
  // bucket) on host threads -- per-part histograms, offsets in (bucket, part) order -- and, in the same scatter, what the track
  // of every RANK brings: its first-camera key and its fixed / non-fixed residual blocks.
  std::vector<int64_t> cnt_main(h->np + 1, 0), cnt_fix(h->np + 1, 0);   // (offsets indexed by track rank, after the running sums)
  std::vector<int> skey(h->np);                                         // run boundaries of the fused plan follow the first-camera key
  {
    const int maxkey = maxkey_all.load();
    struct Ranked { int q, key, nfix, len; };   // one 16-byte record per rank: the scatter is ONE random write per track
    RawArray<Ranked> rk((size_t)h->np);
    auto place = [&](int64_t r, int q) { rk[(size_t)r] = Ranked{q, pkey[q], nfix[q], toff[q + 1] - toff[q]}; };
    auto unpack = [&]() {   // ... and the arrays the later passes read come out of a sequential pass
      host_chunks(h->np, [&](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r) {
          const Ranked& e = rk[(size_t)r];
          porder[r] = e.q; skey[r] = e.key; cnt_fix[r + 1] = e.nfix; cnt_main[r + 1] = e.len - e.nfix;
        }
      });
    };
    if (maxkey >= 0 && (int64_t)maxkey < 8 * (int64_t)h->np + 1024) {
      const int nb = maxkey + 2;
      int parts = host_part_count(h->np, 32768);
      if ((int64_t)parts * nb > ((int64_t)1 << 24)) parts = 1;
      const int64_t per = ((int64_t)h->np + parts - 1) / parts;
      std::vector<int> head((size_t)parts * nb, 0);
      auto bucket = [&](int q) { return skey_pt[q] == std::numeric_limits<int>::max() ? nb - 1 : skey_pt[q]; };
      host_parts(parts, true, [&](int t) {
        int* hh = head.data() + (size_t)t * nb;
        for (int64_t q = t * per; q < std::min<int64_t>(h->np, (t + 1) * per); ++q) hh[bucket((int)q)]++;
      });
      int run = 0;
      for (int bk = 0; bk < nb; ++bk)
        for (int t = 0; t < parts; ++t) { int& c = head[(size_t)t * nb + bk]; const int n = c; c = run; run += n; }
      host_parts(parts, true, [&](int t) {
        int* hh = head.data() + (size_t)t * nb;
        for (int64_t q = t * per; q < std::min<int64_t>(h->np, (t + 1) * per); ++q) place(hh[bucket((int)q)]++, (int)q);
      });
    } else {
      std::stable_sort(porder.begin(), porder.end(), [&](int x, int y) { return skey_pt[x] < skey_pt[y]; });
      for (int r = 0; r < h->np; ++r) place(r, porder[r]);
    }
    unpack();
  }
  tick("  structure: sort tracks");
  for (int r = 0; r < h->np; ++r) { cnt_fix[r + 1] += cnt_fix[r]; cnt_main[r + 1] += cnt_main[r]; }   // ... as running sums
  tick("    permutation: counts");
  h->nobs_main = cnt_main[h->np];
  if (!h->perm.resize((size_t)std::max<int64_t>(1, h->nobs), true)) return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %lld observations failed", (long long)h->nobs);
  // The sorted observation arrays are staged in pinned blocks of the library's host cache: 24 bytes per observation of
  // fresh pageable vectors cost more in page faults than the gather itself, and the copies below run as plain DMA.  They
  // are filled in the pass that lays out the permutation -- a track's observations are read where they lie in the input
  // (one run of it when the input comes track by track) instead of through 3 M random reads of a separate gather pass.
  HBuf<double2> uv, si;
  HBuf<int> ocam_b, opt_b, sred_b;
  if (!uv.resize((size_t)std::max<int64_t>(1, h->nobs), true) || !ocam_b.resize((size_t)std::max<int64_t>(1, h->nobs), true) ||
      !opt_b.resize((size_t)std::max<int64_t>(1, h->nobs), true) || !sred_b.resize((size_t)std::max<int64_t>(1, h->nobs_main), true) ||
      (p->obs_sqrt_info && !si.resize((size_t)std::max<int64_t>(1, h->nobs), true)))
    return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "pinned staging of %lld observations failed", (long long)h->nobs);
  if (!p->obs_sqrt_info) si.n = 0;
  int* const ocam = ocam_b.data();
  int* const opt = opt_b.data();
  int* const sred = sred_b.data();   // participating camera of a non-fixed observation (-1: constant camera and group)
  host_chunks(h->np, [&](int64_t r0, int64_t r1) {   // observations of a track keep their input order
    constexpr int kAhead = 12;   // the tracks of consecutive ranks lie anywhere in the input: their lines are requested ahead
    for (int64_t r = r0; r < r1; ++r) {
      if (r + 2 * kAhead < r1) __builtin_prefetch(&toff[porder[r + 2 * kAhead]]);
      if (r + kAhead < r1) {
        const int qn = porder[r + kAhead];
        if (tobs) __builtin_prefetch(&tobs[toff[qn]]);
        else {
          const size_t i0 = (size_t)toff[qn];
          __builtin_prefetch(p->obs_uv + 2 * i0); __builtin_prefetch(p->obs_uv + 2 * i0 + 8);
          __builtin_prefetch(p->obs_cam + i0); __builtin_prefetch(&fixed[i0]);
          if (p->obs_sqrt_info) { __builtin_prefetch(p->obs_sqrt_info + 2 * i0); __builtin_prefetch(p->obs_sqrt_info + 2 * i0 + 8); }
        }
      }
      const int q = porder[r];
      int64_t m = cnt_main[r], f = h->nobs_main + cnt_fix[r];
      for (int k = toff[q]; k < toff[q + 1]; ++k) {
        const int i = tobs ? tobs[k] : k;
        const int64_t s2 = fixed[i] ? f++ : m++;
        h->perm[s2] = i;
        uv[s2] = make_double2(p->obs_uv[2 * (size_t)i], p->obs_uv[2 * (size_t)i + 1]);
        if (p->obs_sqrt_info) si[s2] = make_double2(p->obs_sqrt_info[2 * (size_t)i], p->obs_sqrt_info[2 * (size_t)i + 1]);
        ocam[s2] = p->obs_cam[i]; opt[s2] = q;
        if (!fixed[i]) sred[s2] = h->cam_part[p->obs_cam[i]];
      }
    }
  });
  tick("    permutation: fill");
  // their uploads start now and run under the rest of the plan construction (pinned sources: nothing waits here; a block that
  // goes back to the host cache on an early return is tagged with an event on this stream, see pool_scope above)
#define UPP(buf, src, cnt, pin) do { rc = h->buf.upload(src, cnt, h->stream, pin); if (rc) return rc; } while (0)
  UPP(obs_uv, uv.data(), (size_t)h->nobs, uv.pinned()); UPP(obs_si, si.data(), si.n, si.pinned());
  UPP(obs_cam, ocam, (size_t)h->nobs, ocam_b.pinned()); UPP(obs_pt, opt, (size_t)h->nobs, opt_b.pinned());
#undef UPP
  // wave tiles: <= 64 observations, never splitting a track
  std::vector<int> tstart, tcount, tkey;
  std::vector<int> l_obs, l_slot, l_start(1, 0), l_pt;  // long tracks (> 64 observations): slow path
  auto build_tiles = [&](const std::vector<int64_t>& off, int64_t base, bool allow_long) -> int {
    int64_t cur0 = 0, curlen = 0;
    int curkey = 0;
    for (int q = 0; q < h->np; ++q) {
      const int64_t L = off[q + 1] - off[q];
      if (L == 0) continue;
      if (L > 64) {
        if (!allow_long) {  // fixed (all-constant) blocks: any split is fine, no per-track sums needed
          if (curlen) { tstart.push_back((int)(base + cur0)); tcount.push_back((int)curlen); tkey.push_back(curkey); curlen = 0; }
          for (int64_t c = 0; c < L; c += 64) { tstart.push_back((int)(base + off[q] + c)); tcount.push_back((int)std::min<int64_t>(64, L - c)); tkey.push_back(0); }
          continue;
        }
        // tiles are contiguous observation ranges: close the open tile before skipping this track
        if (curlen) { tstart.push_back((int)(base + cur0)); tcount.push_back((int)curlen); tkey.push_back(curkey); curlen = 0; }
        const int slot = (int)l_pt.size();
        l_pt.push_back(porder[q]);
        for (int64_t c = 0; c < L; ++c) { l_obs.push_back((int)(base + off[q] + c)); l_slot.push_back(slot); }
        l_start.push_back((int)l_obs.size());
        continue;
      }
      if (curlen + L > 64) { tstart.push_back((int)(base + cur0)); tcount.push_back((int)curlen); tkey.push_back(curkey); curlen = 0; }
      if (curlen == 0) { cur0 = off[q]; curkey = pkey[porder[q]]; }
      curlen += L;
    }
    if (curlen) { tstart.push_back((int)(base + cur0)); tcount.push_back((int)curlen); tkey.push_back(curkey); }
    return 0;
  };
  // Schur assembly without intrinsics: the fused kernel (ba_fused.hip) unless most of the problem would not fit it
  // (tracks that see a camera twice -- e.g. depth-prior rows -- or more than kFusedMaxCams cameras take the
  // per-observation slow path there); THEIA_HIP_SCHUR_GATHER=1 selects the first-generation gather kernels.
  FusedHost fplan;
  tick("  structure: permutation");
  h->use_fused = (h->ni == 0 || h->fused_bw) && h->nobs_main > 0 && !getenv("THEIA_HIP_SCHUR_GATHER");
  const int fused_max_cams = fused_run_cameras(h->fused_bw);
  if (h->use_fused) {
    std::atomic<long long> misfit{0};
    host_chunks(h->np, [&](int64_t q0, int64_t q1) {   // tracks are independent
      std::vector<int> tc;
      long long mine = 0;
      for (int64_t q = q0; q < q1; ++q) {
        const int64_t L = cnt_main[q + 1] - cnt_main[q];
        if (L < 2 || L > 64) continue;
        tc.clear();
        for (int64_t s = cnt_main[q]; s < cnt_main[q + 1]; ++s) if (sred[s] >= 0) tc.push_back(sred[s]);
        std::sort(tc.begin(), tc.end());
        if ((int)tc.size() > fused_max_cams || std::adjacent_find(tc.begin(), tc.end()) != tc.end()) mine += L;
      }
      misfit += mine;
    });
    if (misfit.load() * 20 > h->nobs_main) h->use_fused = false;
    if (!h->use_fused && h->fused_bw) return kRetryWithoutFusedIntr;   // the keys above speak of participating cameras: start over
  }
  tick("  structure: fit check");
  if (h->use_fused) {
    // 32 segments of tracks, cut where the first-camera key changes, built on host threads and merged in order (the
    // segment count is fixed: the plan -- and with it the summation order of S -- does not depend on the machine)
    static const int kSegs = getenv("THEIA_HIP_PLAN_SEGS") ? std::max(1, atoi(getenv("THEIA_HIP_PLAN_SEGS"))) : 32;   // (the switch: measurement only)
    std::vector<int> cut{0};
    if (h->np >= (getenv("THEIA_HIP_HOST_CHUNK_MIN") ? 64 : 65536))
      for (int k = 1; k < kSegs; ++k) {
        int q = (int)((int64_t)h->np * k / kSegs);
        while (q < h->np && q > 0 && skey[q] == skey[q - 1]) ++q;
        if (q > cut.back() && q < h->np) cut.push_back(q);
      }
    cut.push_back(h->np);
    std::vector<FusedSegment> segs(cut.size() - 1);
    tick("    fused plan: keys + cuts");
    fplan.obs_lc.assign((size_t)std::max<int64_t>(1, h->nobs_main), 0xff);
    fplan.obs_tl.assign((size_t)std::max<int64_t>(1, h->nobs_main), 0);
    host_parts((int)segs.size(), true, [&](int k) {
      build_fused_segment(h, cnt_main, porder, sred, ocam, skey, cut[k], cut[k + 1], fplan.obs_lc.data(), fplan.obs_tl.data(), segs[k]);
    });
    tick("    fused plan: segments built");
    merge_fused_segments(h, segs, tstart, tcount, tkey, l_obs, l_slot, l_start, l_pt, fplan);
    tick("    fused plan: merged");
    if (h->fused_bw) {
      int n1 = 0, n2 = 0;
      if ((rc = build_sum_items_intr(h, p->cam_group, fplan, &n1, &n2))) return rc;
      h->n_sum_items2 = n2;
      tick("  structure: sum lists (intrinsics)");
    }
    if (fplan.part_doubles > (size_t)std::numeric_limits<int>::max() / 2)
      return set_error(THEIA_HIP_ERR_UNSUPPORTED, "partial-sum buffer of the fused Schur assembly exceeds 32-bit offsets");
  } else {
    build_tiles(cnt_main, 0, true);
  }
  tick("  structure: fused plan / tiles");
  h->ntiles_main = (int)tstart.size();
  tick("    (tiles)");
  // evaluation-only tiles over the long tracks' observations (no per-track sums there)
  h->long_nobs = (int)l_obs.size(); h->long_ntracks = (int)l_pt.size();
  for (int s2 = 0; s2 < h->long_ntracks; ++s2)
    for (int c = l_start[s2]; c < l_start[s2 + 1]; c += 64) {
      tstart.push_back(l_obs[c]); tcount.push_back(std::min(64, l_start[s2 + 1] - c)); tkey.push_back(0);
    }
  h->ntiles_eval = (int)tstart.size();
  build_tiles(cnt_fix, h->nobs_main, false);
  h->ntiles_all = (int)tstart.size();
  hipStream_t st = h->stream;
#define UP(buf, vec) do { rc = h->buf.upload(vec, st); if (rc) return rc; } while (0)
#define AL(buf, cnt) do { rc = h->buf.alloc(cnt); if (rc) return rc; } while (0)
  tick("structure, sort, tiles");
  h->inner = h->opt.use_inner_iterations != 0 && h->nobs_main > 0;
  if (h->inner) {
    // residual blocks that depend on a block: the camera's / the group's / the track's observations among the
    // non-fixed ones [0, nobs_main) of the sorted arrays (depth-prior rows do not depend on the intrinsics)
    const int64_t nm = h->nobs_main;
    // stable counting sorts by camera / by group on host threads: per-part histograms, offsets in (key, part) order
    // (the index lists go into blocks of the pinned host cache and are uploaded from there: no zero-filled 12 MB vectors,
    // no staging copy; a block that goes back to the cache at the end of this scope is tagged with an event on the stream)
    std::vector<int> coff(h->nc + 1, 0), goff(h->ng + 1, 0), toff;
    HBuf<int> cidx, gidx;
    if (!cidx.resize((size_t)std::max<int64_t>(1, nm), true) || !gidx.resize((size_t)std::max<int64_t>(1, nm), true))
      return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "host staging of %lld observations failed", (long long)nm);
    gidx[0] = 0; gidx.n = 1;
    auto is_depth = [&](int64_t s) { return p->obs_kind && p->obs_kind[h->perm[s]]; };
    auto bucket_sort = [&](int nkeys, std::vector<int>& off, HBuf<int>& idx, auto&& key_of) {   // key < 0: not listed
      const int parts = host_part_count(nm, 65536);
      const int64_t per = (nm + parts - 1) / parts;
      std::vector<int> hist((size_t)parts * nkeys, 0);
      host_parts(parts, true, [&](int t) {
        int* hh = hist.data() + (size_t)t * nkeys;
        for (int64_t s = t * per; s < std::min<int64_t>(nm, (t + 1) * per); ++s) { const int k = key_of(s); if (k >= 0) hh[k]++; }
      });
      int run = 0;
      for (int k = 0; k < nkeys; ++k) {
        off[k] = run;
        for (int t = 0; t < parts; ++t) { const int c = hist[(size_t)t * nkeys + k]; hist[(size_t)t * nkeys + k] = run; run += c; }
      }
      off[nkeys] = run;
      idx.n = (size_t)std::max(1, run);
      host_parts(parts, true, [&](int t) {
        int* hh = hist.data() + (size_t)t * nkeys;
        for (int64_t s = t * per; s < std::min<int64_t>(nm, (t + 1) * per); ++s) { const int k = key_of(s); if (k >= 0) idx[hh[k]++] = (int)s; }
      });
    };
    bucket_sort(h->nc, coff, cidx, [&](int64_t s) { return ocam[s]; });
    if (h->ni) bucket_sort(h->ng, goff, gidx, [&](int64_t s) { return is_depth(s) ? -1 : p->cam_group[ocam[s]]; });
    toff.reserve((size_t)h->np + 1);   // the sorted observations of a track are one range: its non-fixed count
    for (int r = 0; r < h->np; ++r) if (cnt_main[r + 1] > cnt_main[r]) toff.push_back((int)cnt_main[r]);
    toff.push_back((int)nm);
    h->in_ntracks = (int)toff.size() - 1;
    UP(in_cam_off, coff); UP(in_grp_off, goff); UP(in_trk_off, toff);
    if ((rc = h->in_cam_idx.upload(cidx.data(), cidx.n, st, cidx.pinned())) || (rc = h->in_grp_idx.upload(gidx.data(), gidx.n, st, gidx.pinned()))) return rc;
    AL(in_cam, (size_t)6 * std::max(1, h->nc)); AL(in_pts, (size_t)4 * std::max(1, h->np));
    AL(in_intr, (size_t)THEIA_MAX_INTRINSICS * std::max(1, h->ng));
    AL(in_scal, 8); AL(in_part, 4 * (size_t)kInnerCostBlocks); AL(in_gate, 4);
    if (!h->use_fused) AL(camrot_cand, (size_t)40 * std::max(1, h->nc));   // the track sweep reads the cameras as k_cam_prep-style blocks (k_inner_cam_blocks)
    if (h->ni && inner_group_wgs(h->ng) > 1) { AL(in_grp_part, (size_t)h->ng * 2 * inner_group_wgs(h->ng) * kInnerGroupSums); AL(in_grp_bar, 2 * (size_t)std::max(1, h->ng) + 2); }
  }
  if (p->obs_kind) {   // depth-prior rows (sorted like the other observation arrays)
    std::vector<uint8_t> okind(h->nobs);
    for (int64_t s = 0; s < h->nobs; ++s) okind[s] = p->obs_kind[h->perm[s]];
    UP(obs_kind, okind);
  }
  UP(tile_start, tstart); UP(tile_count, tcount);
  UP(long_obs_index, l_obs); UP(long_obs_slot, l_slot); UP(long_track_start, l_start); UP(long_track_pt, l_pt);
  AL(long_scratch, (size_t)14 * std::max(1, h->long_ntracks));
  UP(d_cam_red, h->cam_red); UP(d_cam_mask, h->cam_mask); UP(d_pt_const, h->pt_const);
  std::vector<int> gm(p->group_model, p->group_model + h->ng), cg(p->cam_group, p->cam_group + h->nc);
  h->model_mask = 0u;
  for (int g = 0; g < h->ng; ++g) h->model_mask |= 1u << p->group_model[g];
  UP(group_model, gm); UP(cam_group, cg);
  for (int k = 0; k < 2; ++k) { AL(cam[k], (size_t)6 * h->nc); AL(pts[k], (size_t)4 * h->np); AL(intr[k], (size_t)THEIA_MAX_INTRINSICS * h->ng); }
  UP(d_grp_red, h->grp_red); UP(d_grp_free, h->grp_free); UP(d_grp_k, h->grp_k);
  {
    std::vector<unsigned> rf((size_t)std::max(1, h->ngv), 0u);
    int most = 0;
    for (int g = 0; g < h->ng; ++g)
      if (h->grp_red[g] >= 0) { rf[h->grp_red[g]] = h->grp_free[g]; most = std::max(most, __builtin_popcount(h->grp_free[g])); }
    UP(d_red_free, rf);
    const char* force = getenv("THEIA_HIP_INTR_ROWS");
    h->intr_rows = (most <= 4 && !(force && atoi(force) == 10)) ? 4 : 10;
  }
  {
    std::vector<double> ones_i((size_t)THEIA_MAX_INTRINSICS * h->ng, 1.0);
    UP(ones_i, ones_i); UP(scale_i, ones_i);
  }
  AL(colsq_i0, (size_t)THEIA_MAX_INTRINSICS * h->ng); AL(scale_red, (size_t)std::max(1, h->n));
  AL(ones_c, (size_t)6 * h->nc); AL(ones_p, (size_t)h->pd * h->np); AL(scale_c, (size_t)6 * h->nc); AL(scale_p, (size_t)h->pd * h->np);
  for (PoolBuf<double>* b : {&h->ones_c, &h->ones_p, &h->scale_c, &h->scale_p})   // filled on the device
    if (b->n) k_fill_value<<<(unsigned)std::min<size_t>(1024, (b->n + 255) / 256), 256, 0, st>>>(b->p, b->n, 1.0);
  AL(colsq_c0, (size_t)6 * h->nc); AL(colsq_p0, (size_t)h->pd * h->np);
  {
    std::vector<int> a(&kCfgF2S[0][0], &kCfgF2S[0][0] + 24), b(&kCfgMax[0][0], &kCfgMax[0][0] + 24);
    UP(f2s, a); UP(fmaxflag, b);
  }
  const size_t nn = (size_t)h->n * h->n;
  AL(reduce, nn + 3 * (size_t)h->n + SC_COUNT);
  if (h->reduce.n) HIP_TRYR(hipMemsetAsync(h->reduce.p, 0, sizeof(double) * h->reduce.n, st));
  h->rb.base = h->reduce.p; h->rb.count = h->reduce.n;
  h->rb.S = h->reduce.p; h->rb.rhs = h->rb.S + nn; h->rb.colsq = h->rb.rhs + h->n; h->rb.gc = h->rb.colsq + h->n;
  h->rb.scal = h->rb.gc + h->n;
  AL(Vinv, (size_t)(h->pd * (h->pd + 1) / 2) * h->np); AL(gp, (size_t)h->pd * h->np);
  // constant points are never written: the Schur readers rebuild T = W V^-1 from these arrays and need zeros there
  if (h->Vinv.n) HIP_TRYR(hipMemsetAsync(h->Vinv.p, 0, sizeof(double) * h->Vinv.n, st));
  if (h->gp.n) HIP_TRYR(hipMemsetAsync(h->gp.p, 0, sizeof(double) * h->gp.n, st));
  AL(tile_part, (size_t)5 * std::max(1, h->ntiles_all)); AL(scalB, 16); AL(red_part, (size_t)8 * kReduceBlocks);
  AL(chol_work, dense_cholesky_workspace(h->n));
  AL(lm_state, kLmBlockBytes); AL(lm_ctl, sizeof(LmCtl));
  tick("allocations + uploads");
  {
    std::vector<int> pc, pk;
    std::vector<double> pv, pi;
    collect_cam_priors(p, o->prior_mask, h->nc, nullptr, pc, pk, pv, pi);
    h->n_priors = (int)pc.size();
    UP(prior_cam, pc); UP(prior_kind, pk); UP(prior_vec, pv); UP(prior_info, pi);
  }
  {
    // tile co-visibility: two 64-wide tiles of S couple iff a variable track is
    // seen by cameras of both (the Schur complement's block structure)
    const int nt = (h->n + 63) / 64;
    h->tile_adj.assign((size_t)nt * nt, 0);
    if (h->use_fused && fplan.tile_adj.size() == (size_t)nt * nt) {
      h->tile_adj = fplan.tile_adj;   // marked track by track while the fused plan was built (same rule as below)
    } else {
    std::vector<int64_t> off(h->np + 1, 0);
    for (int64_t i = 0; i < h->nobs; ++i)
      if (h->cam_red[p->obs_cam[i]] >= 0 && !h->pt_const[p->obs_pt[i]]) off[p->obs_pt[i] + 1]++;
    for (int q = 0; q < h->np; ++q) off[q + 1] += off[q];
    std::vector<int> rcs(off[h->np]);
    {
      std::vector<int64_t> fill(off.begin(), off.end() - 1);
      for (int64_t i = 0; i < h->nobs; ++i) {
        const int rcam = h->cam_red[p->obs_cam[i]];
        if (rcam >= 0 && !h->pt_const[p->obs_pt[i]]) rcs[fill[p->obs_pt[i]]++] = rcam;
      }
    }
    std::vector<int> tl;
    for (int q = 0; q < h->np; ++q) {
      tl.clear();
      for (int64_t k = off[q]; k < off[q + 1]; ++k) {
        const int s0 = h->ni + 6 * rcs[k];
        tl.push_back(s0 / 64);
        if ((s0 + 5) / 64 != s0 / 64) tl.push_back((s0 + 5) / 64);
      }
      std::sort(tl.begin(), tl.end());
      tl.erase(std::unique(tl.begin(), tl.end()), tl.end());
      for (int a : tl) for (int b : tl) h->tile_adj[(size_t)a * nt + b] = 1;
    }
    }
    // a variable camera's own 6 x 6 block is written whether or not any of its tracks is variable (F^T F, priors):
    // its tile(s), and the off-diagonal tile when its rows straddle a 64-row boundary, always belong to the plan
    for (int rcam = 0; rcam < h->ncv; ++rcam) {
      const int s0 = h->ni + 6 * rcam, a = s0 / 64, b = (s0 + 5) / 64;
      h->tile_adj[(size_t)a * nt + a] = 1;
      h->tile_adj[(size_t)b * nt + b] = 1;
      h->tile_adj[(size_t)a * nt + b] = h->tile_adj[(size_t)b * nt + a] = 1;
    }
    // which tile columns THIS problem (a rank's shard) writes into: cameras it observes (any point, constant ones included:
    // their F^T F lands on the diagonal) or holds a prior for.  The distributed K3 of a sharded solve asks for it (sync_plan).
    h->tile_touch.assign(nt, 0);
    for (int c = 0; c < h->nc; ++c) {
      const bool prior = p->cam_prior_mask && o->prior_mask && (p->cam_prior_mask[c] & o->prior_mask);
      if ((!cam_used[c] && !prior) || h->cam_red[c] < 0) continue;
      const int s0 = h->ni + 6 * h->cam_red[c];
      h->tile_touch[s0 / 64] = 1; h->tile_touch[(s0 + 5) / 64] = 1;
    }
    // shared intrinsics couple with every camera of their group: treat as dense
    for (int a = 0; a < (h->ni + 63) / 64; ++a)
      for (int b = 0; b < nt; ++b) h->tile_adj[(size_t)a * nt + b] = h->tile_adj[(size_t)b * nt + a] = 1;
    tick("priors + tile adjacency");
    h->plan = chol_plan_create(h->n, h->tile_adj.data());
    tick("K3 plan");
  }
  if (h->ni == 0 && h->ntiles_main > 0 && (rc = build_gather_lists(h, ocam, opt, l_obs, !h->use_fused))) return rc;
  if (h->use_fused) {
    h->n_fruns = (int)fplan.runs.size(); h->n_sum_items = (int)fplan.sum_items.size() / 6 - h->n_sum_items2;
    {   // does every row of the reduced system belong to a camera with a diagonal sum item? (lm_glue_applies: k_schur_sum
        // then writes every entry of rhs / gc / colsq and visits every diagonal entry)
      int ndiag = 0;
      for (int k = 0; k < h->n_sum_items; ++k) ndiag += fplan.sum_items[6 * (size_t)k] == fplan.sum_items[6 * (size_t)k + 1];
      h->sum_covers_n = h->ni == 0 && h->n_sum_items2 == 0 && 6 * ndiag == h->n;
    }
    fplan.tile_trk_end.resize(std::max<size_t>(1, fplan.tile_trk_end.size()));
    if (ctiming) {   // THEIA_HIP_CREATE_TIMING: shape of the fused plan
      std::map<int, std::pair<int, int>> by;   // gp -> (runs, sub-chunks)
      long long nsc = 0;
      for (const FusedRun& r : fplan.runs) { auto& e = by[r.gp]; e.first++; e.second += (r.ntiles + 3) / 4; nsc += (r.ntiles + 3) / 4; }
      fprintf(stderr, "theia_hip fused plan: %zu runs, %lld sub-chunks (%.1f obs each), %zu partial doubles, %d sum items\n",
              fplan.runs.size(), nsc, nsc ? (double)h->nobs_main / nsc : 0.0, fplan.part_doubles, h->n_sum_items);
      fprintf(stderr, "  slice shapes whose dealing missed the closed-form rows (process total): %lld\n", shape_mismatches().load());
      for (auto& kv : by) fprintf(stderr, "  G=%d slices/wave=%d%s: %d runs, %d sub-chunks\n", kv.first & 0xff, (kv.first >> 8) & 0xff, (kv.first & kFusedUnequalSlices) ? " (unequal)" : "", kv.second.first, kv.second.second);
    }
    // THEIA_HIP_PLAN_STATS=<path>: the lane-occupancy model of phase S over this plan (ba_plan_stats.h), as JSON
    if (const char* sp = getenv("THEIA_HIP_PLAN_STATS")) {
      if (*sp && h->fused_bw == 0) {
        const PlanStats ps = fused_plan_occupancy(fplan.runs.data(), (int)fplan.runs.size(), fplan.tgts.data(), tstart.data(), tcount.data(),
                                                  fplan.tile_trk_end.data(), fplan.obs_lc.data(), fplan.obs_tl.data(), fused_tiles_per_subchunk(h->pd));
        if (FILE* f = fopen(sp, "w")) { write_plan_stats_json(f, ps, kFusedRunCostSteps); fclose(f); }
      }
    }
    if (fplan.runs.empty()) fplan.runs.push_back(FusedRun{0, 0, 0, 0, 0, 0, 0, 1 | (1 << 8), 0, 0});
    {   // the workgroups of k_lin_schur take runs from a queue, the most expensive first (cost ~ wave tiles, weighted by the
        // target blocks a wave step covers): the kernel ends when the last run does, and with ~4 runs per workgroup a
        // static round robin left workgroups with one run more than others waiting for them
      std::vector<int> order(fplan.runs.size());
      for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
      const int lanes_tgt = fused_lanes_per_target(h->fused_bw);
      auto cost = [&](int i) { const FusedRun& r = fplan.runs[i]; return (long long)r.ntiles * (64 + lanes_tgt * r.ntgt); };
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
      UP(frun_order, order);
      AL(frun_next, 2);
    }
    fplan.stage.resize(std::max<size_t>(1, fplan.stage.size()));
    UP(fruns, fplan.runs); UP(frun_cams, fplan.cams); UP(frun_stage, fplan.stage); UP(frun_tgt, fplan.tgts); UP(obs_lc, fplan.obs_lc); UP(obs_tl, fplan.obs_tl);
    UP(tile_trk_end, fplan.tile_trk_end); UP(sum_items, fplan.sum_items); UP(sum_src, fplan.sum_src);
    AL(fpart, std::max<size_t>(1, fplan.part_doubles));
    AL(camrot, (size_t)40 * std::max(1, h->nc)); AL(camrot_cand, (size_t)40 * std::max(1, h->nc)); AL(camdir, (size_t)12 * std::max(1, h->nc));
  }
  if (h->ni > 0 && !h->use_fused && h->ntiles_main > 0 && (rc = build_gather_lists_intr(h, p, ocam, opt, l_obs))) return rc;
#undef UP
#undef AL
  tick("gather lists");
  fill_devproblem(h);
  rc = upload_parameters(h, p);
  if (rc) return rc;
  tick("parameter upload");
  // fixed cost
  double fc = 0.0, inv = 0.0;
  rc = cost_of_tiles(h, h->ntiles_eval, h->ntiles_all - h->ntiles_eval, h->cam[0].p, h->pts[0].p, &fc, &inv);
  if (rc) return rc;
  if (h->n_priors) {   // priors on constant cameras: residual blocks without variable parameters
    double pf = 0.0;
    HIP_TRYR(hipMemsetAsync(h->scalB.p, 0, sizeof(double) * 16, h->stream));
    launch_cam_priors(h->P, PRIOR_FIXED, h->cam[0].p, nullptr, nullptr, nullptr, nullptr, h->scalB.p, nullptr, h->stream);
    HIP_TRYR(hipStreamSynchronize(h->stream));
    HIP_TRYR(hipMemcpy(&pf, h->scalB.p, sizeof(double), hipMemcpyDeviceToHost));
    fc += pf;
  }
  h->fixed_cost = fc;
  tick("fixed cost");
  *out = guard.release();
  return 0;
}

}  // namespace

extern "C" int theia_hip_ba_create(const theia_ba_problem* p, const theia_ba_options* o, theia_ba_handle* out) {
  debug_sticky("create entry");
  int rc = ba_create_impl(p, o, out, true);
  if (rc == kRetryWithoutFusedIntr) rc = ba_create_impl(p, o, out, false);
  debug_sticky("create exit");
  return rc;
}
