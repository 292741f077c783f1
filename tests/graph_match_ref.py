"""Sequential restatement, in plain Python / numpy, of the global-descriptor image-pair selection for the tests
of csrc/graph_match.hip: the mean pooling of matching/fisher_vector_extractor.cc:56-69 and GraphMatch of matching/graph_match.cc:
48-130.

graph_match_sequential is the reference's loop as it stands: the score lists filled pair by pair, the partial sort of image i's
list when its turn comes, the two sets per image, the a < m emission.  graph_match_rows is the closed form the device evaluates,
row by row from the kNN lists alone.  The tests hold the two against each other and the device against both.

Arithmetic, every operation fixed: pooled = +0, += each feature in order (float32), /= float32(n);
d(a, b) = fmaf chain over the dimensions ascending from +0.0f of (a - b) * (a - b), the float32 subtraction first."""
import numpy as np

from tests.brute_force_matcher_ref import fmaf32

F32 = np.float32


def mean_pool(features):
    """ExtractGlobalDescriptor: a float32 loop over the features in order."""
    features = np.asarray(features, dtype=F32)
    assert features.ndim == 2 and len(features) > 0          # CHECK_GT (:58)
    assert not np.isnan(features).any()                      # CHECK (:64)
    pooled = np.zeros(features.shape[1], dtype=F32)
    for f in features:
        pooled = (pooled + f).astype(F32)
    return (pooled / F32(len(features))).astype(F32)


def distance_matrix(g):
    """d[i, j] as stated above, float32 [N][N]; symmetric bit for bit."""
    g = np.asarray(g, dtype=F32)
    acc = np.zeros((len(g), len(g)), dtype=F32)
    for c in range(g.shape[1]):
        diff = (g[:, c][:, None] - g[:, c][None, :]).astype(F32)
        acc = fmaf32(diff, diff, acc)
    return acc


def knn_lists(d, k):
    """Per image the k nearest others under (distance, index) ascending: (index [N][k] int32, distance [N][k])."""
    n = len(d)
    k = max(0, min(n - 1, k))
    index = np.zeros((n, k), np.int32); dist = np.zeros((n, k), d.dtype)
    for i in range(n):
        order = sorted((j for j in range(n) if j != i), key=lambda j: (float(d[i, j]), j))[:k]
        index[i] = order
        dist[i] = d[i, order]
    return index, dist


def graph_match_sequential(d, num_nearest_neighbors):
    """The reference's loop on a distance matrix d (d[i, j] is read for i < j only, and serves both images, :69-75).
    Returns the sorted list of selected (a, m), a < m."""
    n = len(d)
    k = min(n - 1, num_nearest_neighbors)
    scores = [[] for _ in range(n)]
    ranked = {}
    expanded = {}
    for i in range(n):
        for j in range(i + 1, n):
            s = d[i, j]
            scores[i].append((float(s), j))
            scores[j].append((float(s), i))
        scores[i].sort()                                     # partial_sort of pair<float, int>: only the first k are read
        for t in range(max(k, 0)):
            second = scores[i][t][1]
            for neighbour in ranked.setdefault(second, set()):
                expanded.setdefault(neighbour, set()).add(i)
            ranked.setdefault(i, set()).add(second)
            ranked.setdefault(second, set()).add(i)
        scores[i] = []
    out = set()
    for a in set(ranked) | set(expanded):
        for m in ranked.get(a, ()):
            if a < m:
                out.add((a, m))
        for m in expanded.get(a, ()):
            if a < m:
                out.add((a, m))
    return sorted(out)


def graph_match_rows(knn_index):
    """The closed form, from the kNN lists alone: (sorted pairs, number of ranked pairs)."""
    n = len(knn_index)
    knn = [[int(s) for s in row] for row in knn_index]
    inv = [[] for _ in range(n)]
    for y in range(n):
        for x in knn[y]:
            inv[x].append(y)
    pairs = []
    num_ranked = 0
    for a in range(n):
        row = set(); ranked = set()
        for s in knn[a]:
            if s > a:
                row.add(s); ranked.add(s)
            row.update(i for i in inv[s] if i > a)
        for s in inv[a]:
            if s > a:
                row.add(s); ranked.add(s)
            row.update(i for i in inv[s] if i > a and i > s)
        pairs.extend((a, i) for i in sorted(row))
        num_ranked += len(ranked)
    return pairs, num_ranked


def graph_match(g, num_nearest_neighbors):
    """Descriptors in, everything the device returns out: (pairs, knn_index, knn_distance) through the literal loop."""
    d = distance_matrix(g)
    index, dist = knn_lists(d, num_nearest_neighbors)
    return graph_match_sequential(d, num_nearest_neighbors), index, dist
