"""Sequential restatement of the track builder's rule (include/theia_hip.h; sfm/track_builder.cc:62-77, :156-209,
math/graph/connected_components.h:87-119, reconstruction.cc:314-351) for the tests of csrc/track_builder.hip.  Written from the
rule, not from the device code: ONE dict union-find over the edges in input order under the cap, then the rules on the
components.  No part of it knows about uncapped components except the two stats fields that count them.

  1. a node is (view, feature), id = feat_off[view] + feature; an edge is one match, in pair order, then match order
  2. per edge: new endpoints become components of size 1; if the endpoints share a component, or size(a) + size(b) > max, nothing;
     otherwise the components merge
  3. a component of fewer than min nodes is dropped (counted before rule 4)
  4. of a component's features in one view the lowest feature index is kept, the others are inconsistent
  5. min < 2, max <= 0, an edge inside one view: refused
  orders: tracks by their smallest node id ascending; a track's observations by node id ascending."""
import bisect

import numpy as np

STATS = ("num_nodes", "num_components", "num_oversized_components", "num_replayed_correspondences", "num_small_components",
         "num_inconsistent_features", "num_tracks", "num_observations")


class Refused(ValueError):
    """what the library answers with THEIA_HIP_ERR_INVALID_ARGUMENT"""


def edge_list(feat_off, pair_view1, pair_view2, match_off, feature1, feature2):
    """The edges as (node1, node2) int64 rows in input order; Refused for what the rule refuses."""
    feat_off = np.asarray(feat_off, np.int64); match_off = np.asarray(match_off, np.int64)
    pv1 = np.asarray(pair_view1, np.int64); pv2 = np.asarray(pair_view2, np.int64)
    nv = len(feat_off) - 1
    if feat_off[0] != 0 or match_off[0] != 0 or (np.diff(feat_off) < 0).any() or (np.diff(match_off) < 0).any():
        raise Refused("offsets")
    if feat_off[-1] >= 2 ** 31:
        raise Refused("too many features")
    if len(pv1) and (min(pv1.min(), pv2.min()) < 0 or max(pv1.max(), pv2.max()) >= nv):
        raise Refused("view index out of range")
    counts = np.diff(match_off)
    if ((pv1 == pv2) & (counts > 0)).any():
        raise Refused("an edge inside one view")
    m = int(match_off[-1])
    f1 = np.asarray(feature1, np.int64)[:m]; f2 = np.asarray(feature2, np.int64)[:m]
    v1 = np.repeat(pv1, counts); v2 = np.repeat(pv2, counts)
    n1 = np.diff(feat_off)[v1] if m else f1; n2 = np.diff(feat_off)[v2] if m else f2
    if m and ((f1 < 0) | (f1 >= n1) | (f2 < 0) | (f2 >= n2)).any():
        raise Refused("feature index outside its view")
    return np.column_stack([feat_off[v1] + f1, feat_off[v2] + f2]) if m else np.zeros((0, 2), np.int64)


def capped_components(edges, max_len):
    """Rule 2 over (a, b) pairs in order: {root: sorted node list}."""
    parent, size = {}, {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        if a not in parent:
            parent[a] = a; size[a] = 1
        if b not in parent:
            parent[b] = b; size[b] = 1
        ra, rb = find(a), find(b)
        if ra == rb or size[ra] + size[rb] > max_len:
            continue
        if size[ra] < size[rb]:
            ra, rb = rb, ra
        parent[rb] = ra
        size[ra] += size[rb]
    comps = {}
    for n in parent:
        comps.setdefault(find(n), []).append(n)
    return {min(c): sorted(c) for c in comps.values()}


def build_tracks(feat_off, pair_view1, pair_view2, match_off, feature1, feature2, min_track_length=2, max_track_length=50):
    """(track_off, obs_view, obs_feature, obs_track, stats) as theia_hip_build_tracks returns them."""
    if min_track_length < 2 or max_track_length <= 0:
        raise Refused("track lengths")
    feat_off = np.asarray(feat_off, np.int64)
    edges = edge_list(feat_off, pair_view1, pair_view2, match_off, feature1, feature2).tolist()
    comps = capped_components(edges, max_track_length)
    starts = feat_off.tolist()
    view_of = lambda node: bisect.bisect_right(starts, node) - 1
    track_off, obs_view, obs_feature, obs_track = [0], [], [], []
    small = inconsistent = 0
    for first in sorted(comps):
        nodes = comps[first]
        if len(nodes) < min_track_length:
            small += 1
            continue
        seen = set()
        for n in nodes:                       # ascending node id: by view, then feature
            v = view_of(n)
            if v in seen:
                inconsistent += 1
                continue
            seen.add(v)
            obs_view.append(v); obs_feature.append(n - starts[v]); obs_track.append(len(track_off) - 1)
        track_off.append(len(obs_view))
    # the two counts of the route through the replay, from a run without the cap
    free = capped_components(edges, float("inf"))
    label = {n: first for first, nodes in free.items() for n in nodes}
    big = {first for first, nodes in free.items() if len(nodes) > max_track_length}
    stats = dict(num_nodes=len(label), num_components=len(free), num_oversized_components=len(big),
                 num_replayed_correspondences=sum(1 for a, _ in edges if label[a] in big), num_small_components=small,
                 num_inconsistent_features=inconsistent, num_tracks=len(track_off) - 1, num_observations=len(obs_view))
    return (np.asarray(track_off, np.int64), np.asarray(obs_view, np.int32), np.asarray(obs_feature, np.int32),
            np.asarray(obs_track, np.int32), stats)


def csr(edges_by_pair):
    """[((view1, view2), [(feature1, feature2), ...]), ...] -> (pair_view1, pair_view2, match_off, feature1, feature2)"""
    pv1 = np.array([p[0][0] for p in edges_by_pair], np.int32); pv2 = np.array([p[0][1] for p in edges_by_pair], np.int32)
    match_off = np.zeros(len(edges_by_pair) + 1, np.int64)
    match_off[1:] = np.cumsum([len(p[1]) for p in edges_by_pair])
    flat = [m for p in edges_by_pair for m in p[1]]
    f1 = np.array([m[0] for m in flat], np.int32); f2 = np.array([m[1] for m in flat], np.int32)
    return pv1, pv2, match_off, f1, f2


def tracks_as_sets(feat_off, track_off, obs_view, obs_feature):
    """the tracks as a sorted list of tuples of (view, feature), for assertions that read like the table of cases"""
    return sorted(tuple((int(obs_view[i]), int(obs_feature[i])) for i in range(track_off[t], track_off[t + 1]))
                  for t in range(len(track_off) - 1))
