// view_graph_device.h -- the device side of view_graph_plan.h for the stages that walk a view graph
// (rotation_averaging.hip, lud_positions.hip, linear_rotations.hip, nonlinear_rotations.hip, nonlinear_positions.hip): the owner that uploads the
// plan's lists once, the struct of their pointers that the kernels take by value, and the device idioms these stages
// share -- the second stage of a block-partial sum, the walk of one wavefront over a free view's edges, the shrinkage
// of the L1 ADMMs.
#pragma once
#include "device_util.h"
#include "view_graph_plan.h"
#include "wave_reduce.h"

namespace thip {

// The lists of view_graph_plan.h on the device, and the edges as (first view, second view).  m free views, P pairs.
struct ViewGraphLists {
  int m, P;
  const int *idx, *free_view, *inc_off, *inc, *pair_off, *pair_edge;
  const int2 *pair_rc, *edges;
};

struct DeviceViewGraph {
  DevBuf<int> idx, free_view, inc_off, inc, pair_off, pair_edge;
  DevBuf<int2> pair_rc, edges;
  ViewGraphLists lists{};

  // edges: [E][2] of n views
  int up(const ViewGraphPlan& g, const int32_t* edges_host, int E, int n) {
    int rc;
    if ((rc = edges.up(edges_host, E)) || (rc = idx.up(g.idx.data(), n)) || (rc = free_view.up(g.free_view.data(), g.m)) ||
        (rc = inc_off.up(g.inc_off.data(), (size_t)g.m + 1)) || (rc = inc.up(g.inc.data(), g.inc.size())) ||
        (rc = pair_off.up(g.pair_off.data(), g.pair_off.size())) || (rc = pair_edge.up(g.pair_edge.data(), g.pair_edge.size())) ||
        (rc = pair_rc.up(g.pair_rc.data(), g.pair_rc.size())))
      return rc;
    lists = ViewGraphLists{g.m, g.P, idx.p, free_view.p, inc_off.p, inc.p, pair_off.p, pair_edge.p, pair_rc.p, edges.p};
    return 0;
  }
};

// Second stage of a reduction: the sum over the nblk blocks of part[block][c] (ncol columns), in every thread -- a
// strided sum per thread, then block_sum: one workgroup, fixed order.
template <int THREADS>
__device__ __forceinline__ double block_sum_column(const double* __restrict__ part, int nblk, int ncol, int c, double* red) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += THREADS) s += part[(size_t)b * ncol + c];
  return block_sum<THREADS>(s, red);
}

// out[c] = sum over blocks of part[block][c]; one workgroup.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_sum_partials(const double* __restrict__ part, int nblk, int ncol,
                                                          double* __restrict__ out) {
  __shared__ double red[THREADS];
  for (int c = 0; c < ncol; ++c) {
    const double s = block_sum_column<THREADS>(part, nblk, ncol, c, red);
    if (threadIdx.x == 0) out[c] = s;
  }
}

// One wavefront per free view, kViewsPerBlock views per workgroup of 256: lane l takes the view's incident edges
// l, l + 64, .. in order and calls f(edge, plus_side), plus_side = the view is the edge's second view.  The sums over
// the lanes (wave_sum_butterfly) stay with the caller.
constexpr int kViewsPerBlock = 256 / 64;
template <class F>
__device__ __forceinline__ void for_each_incident_edge(const ViewGraphLists& g, int v, int lane, F&& f) {
  for (int k = g.inc_off[v] + lane; k < g.inc_off[v + 1]; k += 64) f(g.inc[k] >> 1, (g.inc[k] & 1) != 0);
}

// Shrinkage of the L1 ADMMs: sign(v) max(|v| - kappa, 0).
__device__ __forceinline__ double soft_threshold(double v, double kappa) {
  return fmax(0.0, v - kappa) - fmax(0.0, -v - kappa);
}

}  // namespace thip
