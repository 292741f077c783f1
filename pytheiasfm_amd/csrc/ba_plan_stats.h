// ba_plan_stats.h -- lane-occupancy model of phase S of k_lin_schur (ba_fused.hip) over a finished fused plan: what
// fused_phase_s will issue, run by run, computed on the host from the arrays the kernel reads.  Plain C++ (no device
// code, no HIP header): ba_plan.hip writes it as JSON when THEIA_HIP_PLAN_STATS=<path> is set, and
// tests/plan_occupancy_check.cpp drives it on a hand-built plan.  (The run construction chooses a run's slices on a
// cheaper count of its own, the slot ROWS of its sub-chunks -- every row with a track is one step here.)
//
// The kernel's rule (ba_fused.hip, "phase-S role"): a workgroup of `nwv` waves walks the track slots t of a sub-chunk
// (`tps` wave tiles); with G == 1 a wave serves PS track slices per step -- slice g of wave wv takes slot
// t = base + wv PS + g, base = 0, nwv PS, 2 nwv PS, ... < ntr -- and lane `off_g + k` of the slice owns target k < w_g.
// With G in {2, 4} a group of G waves serves one slot per step, t = base + wv / G, and wave wv owns the targets
// 64 (wv % G) .. + 63.  A wave runs the 108-FMA body of a step on all 64 lanes as soon as ONE lane finds both cameras
// of its target in the slot's camera mask; otherwise the step is skipped.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ba_fused_slices.h"

namespace thip {

struct PlanRunStats {
  int ntgt = 0, W = 0, G = 1, PS = 1, unequal = 0, tiles = 0, obs = 0, tracks = 0;
  long long steps = 0, skipped = 0;   // wave steps of fused_phase_s that run the FMA body / that skip it
  // lanes of the steps that run: 64 steps = useful + idle_shape + idle_sparsity
  long long useful = 0;          // (slot, target) items: the slot's track has both cameras of the lane's target
  long long idle_shape = 0;      // lanes that own no target, and lanes of a slice whose slot holds no track
  long long idle_sparsity = 0;   // lanes that own a target the slot's track does not have
  void add(const PlanRunStats& o) {
    tiles += o.tiles; obs += o.obs; tracks += o.tracks; steps += o.steps; skipped += o.skipped;
    useful += o.useful; idle_shape += o.idle_shape; idle_sparsity += o.idle_sparsity;
  }
};
struct PlanStats {
  std::vector<PlanRunStats> runs;
  PlanRunStats total;
};

// lane offset and width of the slices of a G == 1 run (equal slices: 64 / PS lanes each, the run's ntgt targets in front)
inline int fused_run_slices(int gp, int ntgt, const unsigned short* after_targets, int (&off)[kFusedMaxSlices], int (&wid)[kFusedMaxSlices]) {
  const int PS = std::min(kFusedMaxSlices, std::max(1, (gp >> 8) & 0xff));
  for (int g = 0; g < PS; ++g) {
    if (gp & kFusedUnequalSlices) { off[g] = after_targets[g] & 0xff; wid[g] = after_targets[g] >> 8; }
    else { off[g] = g * (64 / PS); wid[g] = std::min(64 / PS, ntgt); }
  }
  return PS;
}

// Run: FusedRun (ba_kernels.h) or any struct with its tile0 / ntiles / W / tgt_off / ntgt / gp.
//   tgts          frun_tgt: la | lb << 8 per target, a run's slice list behind its targets when gp says so
//   tile_start / tile_count   observation range of a wave tile;  tile_trk_end[last tile of a sub-chunk] = its track slots
//   obs_lc / obs_tl           per observation: local camera (0x80 set: a constant camera, no bit in the mask) / track slot
template <class Run>
PlanStats fused_plan_occupancy(const Run* runs, int nruns, const unsigned short* tgts, const int* tile_start, const int* tile_count,
                               const int* tile_trk_end, const uint8_t* obs_lc, const uint8_t* obs_tl, int tps, int nwv = 4) {
  PlanStats out;
  out.runs.resize((size_t)std::max(0, nruns));
  std::vector<unsigned> mask, filled;
  std::vector<unsigned> tb;
  for (int ir = 0; ir < nruns; ++ir) {
    const Run& r = runs[ir];
    PlanRunStats& st = out.runs[ir];
    st.ntgt = r.ntgt; st.W = r.W; st.G = r.gp & 0xff; st.PS = std::max(1, (r.gp >> 8) & 0xff); st.unequal = (r.gp & kFusedUnequalSlices) ? 1 : 0;
    st.tiles = r.ntiles;
    tb.assign((size_t)r.ntgt, 0u);
    for (int k = 0; k < r.ntgt; ++k) { const unsigned us = tgts[r.tgt_off + k]; tb[k] = (1u << (us & 0xff)) | (1u << (us >> 8)); }
    int off[kFusedMaxSlices], wid[kFusedMaxSlices];
    const int G = st.G, PS = G == 1 ? fused_run_slices(r.gp, r.ntgt, tgts + r.tgt_off + r.ntgt, off, wid) : 1;
    int lanes_in_slices = 0;
    for (int g = 0; g < PS && G == 1; ++g) lanes_in_slices += st.unequal ? wid[g] : 64 / PS;
    for (int t0 = 0; t0 < r.ntiles; t0 += tps) {
      const int t1 = std::min(r.ntiles, t0 + tps);
      const int ntr = tile_trk_end[r.tile0 + t1 - 1];
      mask.assign((size_t)std::max(1, ntr), 0u); filled.assign((size_t)std::max(1, ntr), 0u);
      for (int t = r.tile0 + t0; t < r.tile0 + t1; ++t)
        for (int s = tile_start[t]; s < tile_start[t] + tile_count[t]; ++s) {
          st.obs++;
          if (obs_tl[s] >= ntr) continue;   // (not a plan the kernel could run)
          if (!filled[obs_tl[s]]) { filled[obs_tl[s]] = 1u; st.tracks++; }
          if (!(obs_lc[s] & 0x80)) mask[obs_tl[s]] |= 1u << obs_lc[s];
        }
      auto have = [&](int t, int k0, int k1, long long* hit, long long* miss) {   // targets k0 .. k1-1 against slot t
        for (int k = k0; k < k1; ++k) { if ((mask[t] & tb[k]) == tb[k]) ++*hit; else ++*miss; }
      };
      const int tstride = G == 1 ? nwv * PS : std::max(1, nwv / G);
      for (int wv = 0; wv < nwv; ++wv)
        for (int base = 0; base < ntr; base += tstride) {
          long long hit = 0, miss = 0, shape = 0;
          if (G == 1) {
            shape = 64 - lanes_in_slices;
            for (int g = 0; g < PS; ++g) {
              const int t = base + wv * PS + g, lanes = st.unequal ? wid[g] : 64 / PS;
              if (t < ntr && filled[t]) { have(t, 0, wid[g], &hit, &miss); shape += lanes - wid[g]; }
              else shape += lanes;
            }
          } else {
            const int t = base + wv / G, k0 = std::min(r.ntgt, 64 * (wv % G)), k1 = std::min(r.ntgt, k0 + 64);
            if (t < ntr && filled[t]) { have(t, k0, k1, &hit, &miss); shape = 64 - (k1 - k0); }
            else shape = 64;
          }
          if (hit) { st.steps++; st.useful += hit; st.idle_sparsity += miss; st.idle_shape += shape; }
          else st.skipped++;
        }
    }
    out.total.add(st);
  }
  return out;
}

// The model as JSON: totals, the same per (G, PS) shape, and one row per run.
inline void write_plan_stats_json(FILE* f, const PlanStats& ps, double run_cost_steps) {
  auto frac = [](long long a, long long b) { return b ? (double)a / (double)b : 0.0; };
  auto body = [&](const PlanRunStats& s) {
    fprintf(f, "\"tiles\": %d, \"observations\": %d, \"tracks\": %d, \"steps_issued\": %lld, \"steps_skipped\": %lld, \"lanes_issued\": %lld, "
            "\"lanes_useful\": %lld, \"lanes_idle_shape\": %lld, \"lanes_idle_sparsity\": %lld, \"lane_efficiency\": %.4f, "
            "\"share_idle_shape\": %.4f, \"share_idle_sparsity\": %.4f",
            s.tiles, s.obs, s.tracks, s.steps, s.skipped, 64 * s.steps, s.useful, s.idle_shape, s.idle_sparsity, frac(s.useful, 64 * s.steps),
            frac(s.idle_shape, 64 * s.steps), frac(s.idle_sparsity, 64 * s.steps));
  };
  fprintf(f, "{\n \"model\": \"phase S of k_lin_schur: wave steps that run the FMA body x 64 lanes against (track, target) items\",\n");
  fprintf(f, " \"runs\": %zu, \"run_cost_steps\": %.1f, \"objective_steps\": %.1f,\n \"total\": {", ps.runs.size(), run_cost_steps,
          (double)ps.total.steps + run_cost_steps * (double)ps.runs.size());
  body(ps.total);
  fprintf(f, "},\n \"by_shape\": [");
  std::vector<std::pair<int, PlanRunStats>> by;   // key G | PS << 8 | unequal << 16, in order of first appearance
  std::vector<int> nby;
  for (const PlanRunStats& s : ps.runs) {
    const int key = s.G | (s.PS << 8) | (s.unequal << 16);
    size_t k = 0;
    while (k < by.size() && by[k].first != key) ++k;
    if (k == by.size()) { by.push_back({key, PlanRunStats()}); nby.push_back(0); by[k].second.G = s.G; by[k].second.PS = s.PS; by[k].second.unequal = s.unequal; }
    by[k].second.add(s); nby[k]++;
  }
  for (size_t k = 0; k < by.size(); ++k) {
    fprintf(f, "%s\n  {\"G\": %d, \"PS\": %d, \"unequal_slices\": %d, \"runs\": %d, ", k ? "," : "", by[k].second.G, by[k].second.PS, by[k].second.unequal, nby[k]);
    body(by[k].second);
    fprintf(f, "}");
  }
  fprintf(f, "\n ],\n \"run_columns\": [\"ntgt\", \"W\", \"G\", \"PS\", \"unequal_slices\", \"tiles\", \"observations\", \"tracks\", \"steps_issued\", \"steps_skipped\", "
          "\"lanes_useful\", \"lanes_idle_shape\", \"lanes_idle_sparsity\"],\n \"run_rows\": [");
  for (size_t k = 0; k < ps.runs.size(); ++k) {
    const PlanRunStats& s = ps.runs[k];
    fprintf(f, "%s\n  [%d, %d, %d, %d, %d, %d, %d, %d, %lld, %lld, %lld, %lld, %lld]", k ? "," : "", s.ntgt, s.W, s.G, s.PS, s.unequal, s.tiles, s.obs, s.tracks,
            s.steps, s.skipped, s.useful, s.idle_shape, s.idle_sparsity);
  }
  fprintf(f, "\n ]\n}\n");
}

}  // namespace thip
