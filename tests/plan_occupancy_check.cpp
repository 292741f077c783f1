// Stand-alone driver of the fused plan's lane-occupancy model (csrc/ba_plan_stats.h) on a hand-built plan of three runs;
// prints, per run and in total, "steps skipped useful idle_shape idle_sparsity".  tests/test_plan_occupancy_model.py holds the
// counts written out by hand.
#include <cstdio>
#include <vector>

#include "ba_plan_stats.h"

struct Run { int tile0, ntiles, W, tgt_off, ntgt, gp; };

int main() {
  std::vector<unsigned short> tgts;
  std::vector<int> tile_start, tile_count, tile_trk_end;
  std::vector<uint8_t> lc, tl;
  auto all_pairs = [&](int W) { for (int a = 0; a < W; ++a) for (int b = 0; b <= a; ++b) tgts.push_back((unsigned short)(a | (b << 8))); };
  auto obs = [&](int slot, std::initializer_list<int> cams) { for (int c : cams) { lc.push_back((uint8_t)c); tl.push_back((uint8_t)slot); } };
  auto tile = [&](size_t first_obs, int slots) { tile_start.push_back((int)first_obs); tile_count.push_back((int)(lc.size() - first_obs)); tile_trk_end.push_back(slots); };
  std::vector<Run> runs;

  // run A: three cameras, all six targets, two equal slices of 32 lanes; one tile, three tracks in slots 0 .. 2
  runs.push_back(Run{(int)tile_start.size(), 1, 3, (int)tgts.size(), 6, 1 | (2 << 8)});
  all_pairs(3);
  size_t o = lc.size();
  obs(0, {0, 1}); obs(1, {0, 1, 2}); obs(2, {2});
  tile(o, 3);

  // run B: twelve cameras, all 78 targets on a group of two waves; two tiles of one track each
  runs.push_back(Run{(int)tile_start.size(), 2, 12, (int)tgts.size(), 78, 2 | (1 << 8)});
  all_pairs(12);
  o = lc.size(); obs(0, {0, 1}); tile(o, 1);
  o = lc.size(); obs(1, {11}); tile(o, 2);

  // run C: three cameras, six targets, unequal slices of 6, 3 and 1 targets on lanes 0, 6 and 9; one tile, slots 0 .. 3 hold
  // tracks (slot 2 also sees a constant camera), slot 4 is empty
  runs.push_back(Run{(int)tile_start.size(), 1, 3, (int)tgts.size(), 6, 1 | (3 << 8) | thip::kFusedUnequalSlices});
  all_pairs(3);
  tgts.push_back((unsigned short)(0 | (6 << 8))); tgts.push_back((unsigned short)(6 | (3 << 8))); tgts.push_back((unsigned short)(9 | (1 << 8)));
  o = lc.size();
  obs(0, {0, 1, 2}); obs(1, {0, 1}); obs(2, {0, 0x80}); obs(3, {1, 2});
  tile(o, 5);

  const thip::PlanStats ps = thip::fused_plan_occupancy(runs.data(), (int)runs.size(), tgts.data(), tile_start.data(), tile_count.data(),
                                                        tile_trk_end.data(), lc.data(), tl.data(), 4);
  auto row = [](const char* name, const thip::PlanRunStats& s) {
    printf("%s %lld %lld %lld %lld %lld %d %d\n", name, s.steps, s.skipped, s.useful, s.idle_shape, s.idle_sparsity, s.tracks, s.obs);
  };
  row("A", ps.runs[0]); row("B", ps.runs[1]); row("C", ps.runs[2]); row("total", ps.total);
  thip::write_plan_stats_json(stderr, ps, 88.0);
  return 0;
}
