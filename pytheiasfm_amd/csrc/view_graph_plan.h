// view_graph_plan.h -- what the global-pose stages (rotation_averaging.hip, lud_positions.hip, linear_rotations.hip,
// nonlinear_rotations.hip) derive from a view graph on the host before they touch the device: which views are free, and
// the two CSR lists their kernels assemble the Laplacian-shaped system from without atomics.  Host code only.  The first
// two fix a view per connected component (build_view_graph_plan); the third fixes none and leaves out the views without
// edges (it checks its graph itself, with view_graph_components, and calls fill_view_graph_lists), and so does the
// fourth, which also leaves out the views its caller holds.  nonlinear_positions.hip does as the fourth on a graph whose
// nodes are the views and the track points.
// The device side -- the upload of these lists, the struct the kernels take them in, the walk of a free view's incident
// edges -- is view_graph_device.h; this header stays host code only.
//
// The lists, as the kernels read them:
//   inc[inc_off[t] .. inc_off[t + 1])            the edges incident to free view t, in edge order;
//                                                inc[k] = 2 * edge + (1 if t is the edge's second view, the +I side)
//   pair_rc[p] = (a, b), a > b                   the p-th unordered pair of free views joined by an edge, as the (row, column)
//                                                of its block in the lower triangle; pairs ascend by (a, b)
//   pair_edge[pair_off[p] .. pair_off[p + 1])    that pair's edges, in edge order
// An edge from a view to itself is in neither list (its rows of A are zero for the rotations, its position terms cancel
// for the positions); an edge with one fixed end is in its free end's inc only.
#pragma once
#include "theia_hip_internal.h"

#include <algorithm>
#include <numeric>
#include <utility>
#include <vector>

namespace thip {

struct ViewGraphPlan {
  std::vector<int> idx;         // [num_views] view -> free index, -1 for a fixed view
  std::vector<int> free_view;   // [m] free index -> view, in view order
  std::vector<int> inc_off, inc, pair_off, pair_edge;
  std::vector<int2> pair_rc;
  int m = 0, P = 0;             // free views, unordered free-view pairs
};

inline int find_root(std::vector<int>& parent, int v) {
  while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
  return v;
}

// The lists of the free views, those with fix[v] == 0, indexed compactly in view order.  The edges are in range.
inline void fill_view_graph_lists(int n, const std::vector<uint8_t>& fix, int E, const int32_t* edges, ViewGraphPlan* plan) {
  std::vector<int>& idx = plan->idx;
  idx.assign(n, -1);
  plan->free_view.clear();
  for (int v = 0; v < n; ++v) if (!fix[v]) { idx[v] = (int)plan->free_view.size(); plan->free_view.push_back(v); }
  const int m = plan->m = (int)plan->free_view.size();

  std::vector<int>& inc_off = plan->inc_off;
  inc_off.assign(m + 1, 0);
  std::vector<std::pair<int64_t, int>> pe;   // (pair key, edge)
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i == j) continue;
    if (idx[i] >= 0) ++inc_off[idx[i] + 1];
    if (idx[j] >= 0) ++inc_off[idx[j] + 1];
    if (idx[i] >= 0 && idx[j] >= 0) {
      const int a = std::max(idx[i], idx[j]), b = std::min(idx[i], idx[j]);
      pe.emplace_back((int64_t)a * m + b, e);
    }
  }
  for (int v = 0; v < m; ++v) inc_off[v + 1] += inc_off[v];
  plan->inc.resize(inc_off[m]);
  {
    std::vector<int> fill(inc_off.begin(), inc_off.end() - 1);
    for (int e = 0; e < E; ++e) {
      const int i = edges[2 * e], j = edges[2 * e + 1];
      if (i == j) continue;
      if (idx[i] >= 0) plan->inc[fill[idx[i]]++] = 2 * e;
      if (idx[j] >= 0) plan->inc[fill[idx[j]]++] = 2 * e + 1;
    }
  }
  std::sort(pe.begin(), pe.end());   // the (key, edge) entries are unique: a pair's edges stay in edge order
  plan->pair_off.assign(1, 0);
  plan->pair_edge.resize(pe.size());
  plan->pair_rc.clear();
  for (size_t k = 0; k < pe.size(); ++k) {
    if (k == 0 || pe[k].first != pe[k - 1].first) {
      if (k) plan->pair_off.push_back((int)k);
      plan->pair_rc.push_back(make_int2((int)(pe[k].first / m), (int)(pe[k].first % m)));
    }
    plan->pair_edge[k] = pe[k].second;
  }
  plan->pair_off.push_back((int)pe.size());
  plan->P = (int)plan->pair_rc.size();
}

// Checks that every edge names views in range (THEIA_HIP_ERR_INVALID_ARGUMENT otherwise) and gives every view the root of
// its connected component, the component's smallest view.
inline int view_graph_components(int n, int E, const int32_t* edges, std::vector<int>* root) {
  for (int e = 0; e < E; ++e)
    if (edges[2 * e] < 0 || edges[2 * e] >= n || edges[2 * e + 1] < 0 || edges[2 * e + 1] >= n)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "edge %d names a view out of range", e);
  std::vector<int>& parent = *root;
  parent.resize(n);
  std::iota(parent.begin(), parent.end(), 0);
  for (int e = 0; e < E; ++e) {
    const int a = find_root(parent, edges[2 * e]), b = find_root(parent, edges[2 * e + 1]);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  for (int v = 0; v < n; ++v) parent[v] = find_root(parent, v);
  return 0;
}

// What the view-graph prunings (view_graph_pruning.hip) refuse in their pair list: a view out of range, a self-pair, an
// unordered pair named twice -- the conditions view_pair_filters.hip checks with its file-local copy of this function.
inline int check_pairs(int n_views, int n_pairs, const int32_t* pairs) {
  std::vector<uint64_t> keys((size_t)n_pairs);
  for (int e = 0; e < n_pairs; ++e) {
    const int i = pairs[2 * e], j = pairs[2 * e + 1];
    if (i < 0 || i >= n_views || j < 0 || j >= n_views)
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %d names a view out of range", e);
    if (i == j) return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "pair %d names view %d twice", e, i);
    keys[e] = ((uint64_t)std::min(i, j) << 32) | (uint64_t)std::max(i, j);
  }
  std::sort(keys.begin(), keys.end());
  for (int e = 1; e < n_pairs; ++e)
    if (keys[e] == keys[e - 1])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "the pair (%d, %d) is listed twice", (int)(keys[e] >> 32),
                       (int)(keys[e] & 0xFFFFFFFFu));
  return 0;
}

// Checks the edges and builds the plan.  fixed: [n] flags or null; no view flagged: view 0 is fixed.  `word` names a
// fixed view in the error text ("fixed" for rotations, "held" for positions).  THEIA_HIP_ERR_INVALID_ARGUMENT: an edge
// names a view out of range; a connected component has no fixed view (the system would be singular).
inline int build_view_graph_plan(int n, const uint8_t* fixed, int E, const int32_t* edges, const char* word,
                                 ViewGraphPlan* plan) {
  std::vector<int> root;
  if (int rc = view_graph_components(n, E, edges, &root)) return rc;

  std::vector<uint8_t> fix(n, 0);
  bool any = false;
  for (int v = 0; v < n && fixed; ++v) { fix[v] = fixed[v] ? 1 : 0; any = any || fix[v]; }
  if (!any) fix[0] = 1;
  std::vector<uint8_t> anchored(n, 0);
  for (int v = 0; v < n; ++v) if (fix[v]) anchored[root[v]] = 1;
  for (int v = 0; v < n; ++v)
    if (!anchored[root[v]])
      return set_error(THEIA_HIP_ERR_INVALID_ARGUMENT, "view %d lies in a connected component without a %s view", v, word);
  fill_view_graph_lists(n, fix, E, edges, plan);
  return 0;
}

}  // namespace thip
