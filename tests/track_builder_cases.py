"""Match graphs for the track builder's tests: cases whose answer can be read off (the expected tracks are written by hand, never
computed), and the generators of the larger scenes.  A case gives its edges per image pair, ((view1, view2), [(feature1,
feature2), ...]), in input order; every view has FEATURES_PER_VIEW features."""
import numpy as np

from tests import track_builder_ref as ref

FEATURES_PER_VIEW = 4
CHAIN6 = [((v, v + 1), [(0, 0)]) for v in range(5)]    # one feature followed through views 0 .. 5

# name, number of views, pairs, min, max, the tracks as sets of (view, feature), the stats that can be read off
READ_OFF = [
    ("four disjoint matches", 3, [((0, 1), [(0, 0), (1, 1)]), ((1, 2), [(2, 2), (3, 3)])], 2, 50,
     [((0, 0), (1, 0)), ((0, 1), (1, 1)), ((1, 2), (2, 2)), ((1, 3), (2, 3))],
     dict(num_nodes=8, num_components=4, num_small_components=0, num_inconsistent_features=0, num_oversized_components=0)),
    ("chain of three, max 2", 3, [((0, 1), [(0, 0)]), ((1, 2), [(0, 0)])], 2, 2,
     [((0, 0), (1, 0))],      # (2, 0) stays a singleton and is dropped
     dict(num_nodes=3, num_components=1, num_oversized_components=1, num_replayed_correspondences=2, num_small_components=1)),
    ("two features of one view in a component", 3, [((0, 1), [(0, 0), (0, 1)]), ((1, 2), [(2, 0), (2, 1)])], 2, 50,
     [((0, 0), (1, 0)), ((1, 2), (2, 0))],     # (1, 1) and (2, 1) are inconsistent: the lower feature index is kept
     dict(num_nodes=6, num_components=2, num_inconsistent_features=2, num_observations=4)),
    ("chain over six views, max 2", 6, CHAIN6, 2, 2,
     [((0, 0), (1, 0)), ((2, 0), (3, 0)), ((4, 0), (5, 0))],
     dict(num_nodes=6, num_components=1, num_oversized_components=1, num_replayed_correspondences=5, num_small_components=0)),
    ("chain over six views, max 10, min 3, and a separate match", 6, CHAIN6 + [((0, 1), [(1, 1)])], 3, 10,
     [((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0))],
     dict(num_nodes=8, num_components=2, num_oversized_components=0, num_small_components=1)),
    ("three nodes with a repeated view, min 3", 2, [((0, 1), [(0, 0), (0, 1)])], 3, 50,
     [((0, 0), (1, 0))],      # the node count 3 passes min 3; the track has two observations
     dict(num_nodes=3, num_components=1, num_small_components=0, num_inconsistent_features=1, num_observations=2)),
    # a path over four views, max 3: in path order the fourth node is left over; with the middle edge last, two pairs
    ("path of four, max 3, in path order", 4, [((0, 1), [(0, 0)]), ((1, 2), [(0, 0)]), ((2, 3), [(0, 0)])], 2, 3,
     [((0, 0), (1, 0), (2, 0))],
     dict(num_oversized_components=1, num_replayed_correspondences=3, num_small_components=1)),
    ("path of four, max 3, middle edge last", 4, [((0, 1), [(0, 0)]), ((2, 3), [(0, 0)]), ((1, 2), [(0, 0)])], 2, 3,
     [((0, 0), (1, 0)), ((2, 0), (3, 0))],
     dict(num_oversized_components=1, num_replayed_correspondences=3, num_small_components=0)),
]
READ_OFF_IDS = [c[0] for c in READ_OFF]


def read_off_input(case):
    """(feat_off, pair_view1, pair_view2, match_off, feature1, feature2) of a READ_OFF case"""
    _, num_views, pairs, _, _, _, _ = case
    feat_off = FEATURES_PER_VIEW * np.arange(num_views + 1, dtype=np.int64)
    return (feat_off,) + ref.csr(pairs)


def random_match_graph(seed, num_views=12, features=300, points=250, seen=0.5, matched=0.8, outliers=0.02):
    """Every view sees each point with probability `seen`, at a feature index of its own; a point two views share is matched
    with probability `matched`; `outliers` x that many random matches are added per pair; all pairs i < j, the first one
    listed a second time at the end."""
    rng = np.random.default_rng(seed)
    visible = rng.random((num_views, points)) < seen
    feature_of = np.stack([rng.permutation(features)[:points] for _ in range(num_views)])
    pairs = []
    for i in range(num_views):
        for j in range(i + 1, num_views):
            both = np.nonzero(visible[i] & visible[j] & (rng.random(points) < matched))[0]
            edges = [(int(feature_of[i, p]), int(feature_of[j, p])) for p in both]
            edges += [(int(rng.integers(features)), int(rng.integers(features))) for _ in range(int(outliers * len(both)))]
            pairs.append(((i, j), edges))
    pairs.append(pairs[0])
    feat_off = features * np.arange(num_views + 1, dtype=np.int64)
    return (feat_off,) + ref.csr(pairs)


def permute_pairs(graph, seed):
    """the same pairs, each with its matches in their order, in another pair order"""
    feat_off, pv1, pv2, match_off, f1, f2 = graph
    order = np.random.default_rng(seed).permutation(len(pv1))
    pairs = [((int(pv1[k]), int(pv2[k])), list(zip(f1[match_off[k]:match_off[k + 1]].tolist(), f2[match_off[k]:match_off[k + 1]].tolist())))
             for k in order]
    return (feat_off,) + ref.csr(pairs)


def path_graph(num_nodes, seed):
    """one feature followed through num_nodes views, every edge a pair of its own, the pairs shuffled"""
    order = np.random.default_rng(seed).permutation(num_nodes - 1)
    pairs = [((int(v), int(v) + 1), [(0, 0)]) for v in order]
    return (np.arange(num_nodes + 1, dtype=np.int64),) + ref.csr(pairs)


def star_graph(leaves, leaf_views=50):
    """feature 0 of view 0 matched to `leaves` features spread evenly over leaf_views other views"""
    per = leaves // leaf_views
    pairs = [((0, v), [(0, f) for f in range(per)]) for v in range(1, leaf_views + 1)]
    feat_off = np.concatenate([[0, 1], 1 + per * np.arange(1, leaf_views + 1)]).astype(np.int64)
    return (feat_off,) + ref.csr(pairs)


def disjoint_matches(count, seed, shuffle_seed=None):
    """two views of `count` features, feature i of view 0 matched to feature perm[i] of view 1; with shuffle_seed the same
    matches in another order"""
    perm = np.random.default_rng(seed).permutation(count)
    f1 = np.arange(count)
    if shuffle_seed is not None:
        f1 = np.random.default_rng(shuffle_seed).permutation(count)
    feat_off = np.array([0, count, 2 * count], np.int64)
    return (feat_off, np.array([0], np.int32), np.array([1], np.int32), np.array([0, count], np.int64),
            f1.astype(np.int32), perm[f1].astype(np.int32))


def cap_boundary_graph(max_len):
    """feature 0 followed through max_len views (a component of exactly max_len nodes) and feature 1 through max_len + 1 views"""
    pairs = [((v, v + 1), [(0, 0), (1, 1)]) for v in range(max_len - 1)] + [((max_len - 1, max_len), [(1, 1)])]
    return (2 * np.arange(max_len + 2, dtype=np.int64),) + ref.csr(pairs)
