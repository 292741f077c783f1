// ba_fused_slices.h -- how FusedRun::gp (ba_kernels.h) describes unequal track slices; shared by the kernels, the plan builder
// and the host-only plan model (ba_plan_stats.h), so no other header comes with it.
#pragma once

namespace thip {

// gp of a run: G | PS << 8 | kFusedUnequalSlices when the run's slices are listed behind its targets
// (frun_tgt[tgt_off + ntgt + g] = lane offset | width << 8; slice g owns the FIRST `width` targets of the run)
constexpr int kFusedUnequalSlices = 1 << 16;
constexpr int kFusedMaxSlices = 10;

}  // namespace thip
