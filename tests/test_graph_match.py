"""CPU: the global-descriptor image-pair selection on cases whose answer can be read off, the literal loop of
tests/graph_match_ref.py against the closed form the device evaluates, the ABI of theia_hip_mean_pool_descriptors /
theia_hip_graph_match (every refusal that needs no device, the trivial cases) and the host side of the mirror in
pytheiasfm_amd/matching.py.  The device code is tested in tests/test_graph_match_gpu.py.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from tests import graph_match_cases as cases, graph_match_ref as ref

F32 = np.float32


@pytest.mark.parametrize("case", cases.READ_OFF, ids=cases.READ_OFF_IDS)
def test_literal_loop_on_read_off_cases(case):
    _, k, expected = case
    pairs, index, dist = ref.graph_match(cases.read_off_descriptors(case), k)
    assert pairs == expected
    assert ref.graph_match_rows(index)[0] == expected
    assert index.shape == (len(case[0]), min(len(case[0]) - 1, k))


def test_knn_ties_go_to_the_lower_index():
    d = ref.distance_matrix(np.zeros((4, 1), F32))
    index, dist = ref.knn_lists(d, 2)
    assert index.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1]] and not dist.any()


def test_distance_is_symmetric_bit_for_bit_and_a_fmaf_chain():
    g = cases.clustered(9, 33, seed=3)
    d = ref.distance_matrix(g)
    assert np.array_equal(d.view(np.uint32), d.T.view(np.uint32))
    acc = F32(0)
    for c in range(33):
        diff = F32(g[2, c] - g[7, c])
        acc = ref.fmaf32(diff, diff, acc)
    assert d[2, 7].view(np.uint32) == np.asarray(acc, F32).view(np.uint32)
    # the chain is not what a float64 sum rounds to on this input: the order is part of the definition
    plain = ((g.astype(np.float64)[:, None] - g.astype(np.float64)[None]) ** 2).sum(-1).astype(F32)
    assert not np.array_equal(plain, d)


def test_literal_loop_equals_closed_form_on_random_inputs_with_ties():
    """400 small inputs, distances drawn from a handful of values so that the tie rule decides most lists"""
    rng = np.random.default_rng(20)
    differ_from_symmetric_closure = 0
    for trial in range(400):
        n = int(rng.integers(2, 13))
        k = int(rng.integers(1, n + 2))
        upper = np.triu(rng.integers(0, 4, size=(n, n)).astype(F32), 1)
        d = upper + upper.T
        index, _ = ref.knn_lists(d, k)
        sequential = ref.graph_match_sequential(d, k)
        rows, num_ranked = ref.graph_match_rows(index)
        assert sequential == rows, (trial, n, k)
        ranked = {(min(a, int(s)), max(a, int(s))) for a in range(n) for s in index[a]}
        assert num_ranked == len(ranked) and ranked <= set(rows)
        # the dropped a > i entries: the rule is NOT "ranked plus every pair with a common ranked neighbour"
        closure = set(ranked)
        adj = [set() for _ in range(n)]
        for a, b in ranked:
            adj[a].add(b); adj[b].add(a)
        for s in range(n):
            closure |= {(a, b) for a in adj[s] for b in adj[s] if a < b}
        assert set(rows) <= closure
        differ_from_symmetric_closure += set(rows) != closure
    assert differ_from_symmetric_closure > 0


def test_mean_pool_restatement():
    f = np.array([[1, 2], [3, 4], [5, 9]], F32)
    assert ref.mean_pool(f).tolist() == [3.0, 5.0]
    big = np.array([[1e30], [1.0], [-1e30]], F32)
    assert ref.mean_pool(big).tolist() == [0.0]          # the order of the adds is the definition: 1e30 + 1 - 1e30
    assert ref.mean_pool(big[[0, 2, 1]])[0] == F32(1.0) / F32(3.0)


def test_struct_size_and_exported_names():
    from pytheiasfm_amd import _capi as capi
    assert C.sizeof(capi.GraphMatchStats) == 4 * 8
    assert [name for name, _ in capi.GraphMatchStats._fields_] == ["num_nearest_neighbors", "num_ranked_pairs",
                                                                   "num_expanded_pairs", "num_pairs"]
    for name in ("theia_hip_mean_pool_descriptors", "theia_hip_graph_match"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)
    assert sum("graph_match" in s or "mean_pool" in s for s in capi.EXPORTED_SYMBOLS) == 2


def _pool(num_images, feat_off, dim, desc, null=()):
    from pytheiasfm_amd import _capi as capi
    feat_off = np.array(feat_off, np.int64); desc = np.array(desc, F32)
    out = np.full(max(1, num_images) * max(1, dim), -7, F32)
    rc = capi.lib().theia_hip_mean_pool_descriptors(num_images, None if "feat_off" in null else capi.ptr(feat_off, C.c_int64), dim,
                                                    None if "desc" in null else capi.ptr(desc, C.c_float),
                                                    None if "out" in null else capi.ptr(out, C.c_float))
    return rc, out


def _match(num_images, dim, g, k, capacity=8, null=()):
    from pytheiasfm_amd import _capi as capi
    g = np.array(g, F32)
    p1 = np.full(8, -7, np.int32); p2 = np.full(8, -7, np.int32)
    knn_index = np.full(16, -7, np.int32); knn_distance = np.full(16, -7, F32)
    count = C.c_int64(-7)
    stats = capi.GraphMatchStats(num_pairs=-7)
    rc = capi.lib().theia_hip_graph_match(num_images, dim, None if "g" in null else capi.ptr(g, C.c_float), k, capacity,
                                          None if "p1" in null else capi.ptr(p1, C.c_int32),
                                          None if "p2" in null else capi.ptr(p2, C.c_int32),
                                          None if "count" in null else C.byref(count), capi.ptr(knn_index, C.c_int32),
                                          capi.ptr(knn_distance, C.c_float), C.byref(stats))
    untouched = all((a == -7).all() for a in (p1, p2, knn_index, knn_distance))
    return rc, untouched, count.value, stats


def test_pooling_refusals_need_no_device_and_leave_the_output():
    from pytheiasfm_amd import _capi as capi
    bad = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    desc = np.ones((4, 2), F32)
    for args, kw in (((-1, [0], 2, desc), {}),                       # negative size
                     ((2, [0, 2, 4], 0, desc), {}),                  # dim < 1
                     ((2, [0, 2, 4], -2, desc), {}),
                     ((2, [1, 2, 4], 2, desc), {}),                  # feat_off does not start at 0
                     ((2, [0, 3, 2], 2, desc), {}),                  # decreases
                     ((2, [0, 0, 4], 2, desc), {}),                  # an image without features
                     ((2, [0, 4, 4], 2, desc), {}),
                     ((2, [0, 2, 4], 2, desc), dict(null=("feat_off",))),
                     ((2, [0, 2, 4], 2, desc), dict(null=("desc",))),
                     ((2, [0, 2, 4], 2, desc), dict(null=("out",)))):
        rc, out = _pool(*args, **kw)
        assert rc == bad and (out == -7).all(), (args[:3], kw)
        assert capi.lib().theia_hip_last_error()
    rc, out = _pool(0, [0], 2, np.zeros((0, 2), F32))                # no images: nothing to do
    assert rc == 0 and (out == -7).all()
    rc, out = _pool(0, [0], 2, np.zeros((0, 2), F32), null=("feat_off", "desc", "out"))
    assert rc == 0


def test_graph_match_refusals_need_no_device_and_leave_the_outputs():
    from pytheiasfm_amd import _capi as capi
    bad = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    g = np.arange(8, dtype=F32).reshape(4, 2)
    nan = g.copy(); nan[2, 1] = np.nan
    inf = g.copy(); inf[0, 0] = -np.inf
    for args, kw in (((-1, 2, g, 1), {}),
                     ((4, 0, g, 1), {}),
                     ((4, -1, g, 1), {}),
                     ((4, 2, g, -1), {}),                            # num_nearest_neighbors < 0
                     ((4, 2, g, 1), dict(capacity=-1)),
                     ((4, 2, g, 1), dict(null=("g",))),
                     ((4, 2, g, 1), dict(null=("p1",))),
                     ((4, 2, g, 1), dict(null=("p2",))),
                     ((4, 2, g, 1), dict(null=("count",))),
                     ((4, 2, nan, 1), {}),                           # a NaN distance has no place in the order
                     ((4, 2, inf, 1), {}),
                     ((1, 2, nan[2:], 1), {})):
        rc, untouched, count, stats = _match(*args, **kw)
        assert rc == bad and untouched and count == -7 and stats.num_pairs == -7, (args[0], args[1], args[3], kw)


def test_trivial_cases_return_zero_pairs_without_a_device():
    g = np.arange(8, dtype=F32).reshape(4, 2)
    for args, kw, k_out in (((0, 2, g[:0], 5), {}, 0), ((0, 2, g[:0], 5), dict(null=("g",)), 0), ((1, 2, g[:1], 5), {}, 0),
                            ((4, 2, g, 0), {}, 0), ((4, 2, g, 0), dict(capacity=0, null=("p1", "p2")), 0)):
        rc, untouched, count, stats = _match(*args, **kw)
        assert rc == 0 and untouched and count == 0, (args[0], args[3], kw)
        assert (stats.num_nearest_neighbors, stats.num_ranked_pairs, stats.num_expanded_pairs, stats.num_pairs) == (k_out, 0, 0, 0)


def test_mirror_shapes_and_name_ordering(monkeypatch):
    """GraphMatch orients a pair by image INDEX and sorts the list by the pair of NAMES (graph_match.cc:108-128): with names whose
    string order differs from their index order the two show apart.  The device call is replaced by the restatement."""
    from pytheiasfm_amd import matching
    o = matching.FisherVectorExtractor.Options()
    assert (o.num_gmm_clusters, o.max_num_features_for_training) == (16, 100000)
    fv = matching.FisherVectorExtractor(o)
    assert fv.AddFeaturesForTraining([np.zeros(4, F32)]) is None and fv.Train() is True

    def restated(g, k, want_knn=False):
        pairs, index, _ = ref.graph_match(g, k)
        return np.asarray(pairs, np.int32).reshape(-1, 2), {}

    monkeypatch.setattr(matching, "graph_match", restated)
    names = ["d.jpg", "a.jpg", "c.jpg", "b.jpg"]
    got = matching.GraphMatch(names, cases.read_off_descriptors(cases.READ_OFF[1]), 1)
    # index pairs (0,1) (0,2) (0,3) (2,3): the first name is the lower INDEX, also where it is the later string
    assert got == [("c.jpg", "b.jpg"), ("d.jpg", "a.jpg"), ("d.jpg", "b.jpg"), ("d.jpg", "c.jpg")]

    monkeypatch.setattr(matching, "mean_pool_descriptors", lambda descs: np.stack([ref.mean_pool(d) for d in descs]))
    m = matching.BruteForceFeatureMatcher()
    for name, value in zip(names, cases.READ_OFF[1][0]):
        m.AddImage(name, matching.KeypointsAndDescriptors(np.zeros((2, 2)), np.full((2, 1), value, F32)))
    assert m.pairs_to_match_ == []
    assert matching.SelectImagePairsWithGlobalDescriptorMatching(m, 1) == got and m.pairs_to_match_ == got
