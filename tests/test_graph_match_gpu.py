"""GPU: the global-descriptor image-pair selection (csrc/graph_match.hip: the mean pooling of matching/fisher_vector_extractor.cc:
56-69 and GraphMatch, matching/graph_match.cc:48-130) against the literal restatement in tests/graph_match_ref.py and, where the
distances are exact in any order, against plain float64 numpy.  Pairs and kNN indices are integers, kNN distances and pooled
descriptors are compared by their bits: every comparison is equality, no tolerance appears."""
import ctypes as C
import functools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, matching
from tests import graph_match_cases as cases, graph_match_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = {"tied": cases.tied_integers, "hub": cases.hub, "clustered": cases.clustered}
NS = [2, 3, 5, 63, 64, 65, 130, 257]
DIMS = [1, 3, 32, 33, 128]


def ks_of(n):
    return sorted({k for k in (1, 2, 7, n - 2, n - 1, 100) if k >= 0})


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@functools.lru_cache(maxsize=4)
def restated(kind, n, dim):
    """(descriptors, distance matrix, every image's full (distance, index) order): shared by the k of one input, never changed"""
    g = KINDS[kind](n, dim, seed=1000 * n + dim)
    d = ref.distance_matrix(g)
    index, dist = ref.knn_lists(d, n - 1)
    for a in (g, d, index, dist):
        a.setflags(write=False)
    return g, d, index, dist


def check(g, k, d, full_index, full_dist):
    """the device == the literal loop: pairs, kNN lists, kNN distances (bits), and the stats"""
    n = len(g)
    kk = max(0, min(n - 1, k))
    pairs, stats, knn_index, knn_distance = matching.graph_match(g, k, want_knn=True)
    assert knn_index.shape == knn_distance.shape == (n, kk)
    assert np.array_equal(knn_index, full_index[:, :kk])
    assert np.array_equal(bits(knn_distance), bits(full_dist[:, :kk]))
    want = ref.graph_match_sequential(d, k)
    assert pairs.dtype == np.int32 and pairs.tolist() == [list(p) for p in want]
    rows, num_ranked = ref.graph_match_rows(full_index[:, :kk])
    assert rows == want
    assert stats == dict(num_nearest_neighbors=kk, num_ranked_pairs=num_ranked, num_expanded_pairs=len(want) - num_ranked,
                         num_pairs=len(want))
    return pairs


# ------------------------------------------------------------------------------------------------ 1. device vs the literal loop
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", NS)
def test_device_equals_the_literal_loop(n, kind, dim):
    g, d, index, dist = restated(kind, n, dim)
    if kind == "hub" and n > 2 and dim == 128:                       # random directions are near orthogonal there: 10 < 10 sqrt(2)
        assert all(index[i, 0] == n // 2 for i in range(n) if i != n // 2)
    if kind == "tied" and n > 3:
        assert (d[np.triu_indices(n, 1)] == 0).any()              # duplicate images: the tie rule decides
    for k in ks_of(n):
        check(g, k, d, index, dist)


@pytest.mark.parametrize("case", cases.READ_OFF, ids=cases.READ_OFF_IDS)
def test_read_off_cases(case):
    g = cases.read_off_descriptors(case)
    d = ref.distance_matrix(g)
    index, dist = ref.knn_lists(d, len(g) - 1)
    assert check(g, case[1], d, index, dist).tolist() == [list(p) for p in case[2]]


def test_fmaf_order_is_what_the_device_computes():
    """on the clustered input a float64 sum rounded once differs from the chain in some distance: the equality above is about the
    stated order, not about any accurate sum"""
    g, d, _, _ = restated("clustered", 130, 128)
    g64 = g.astype(np.float64)
    plain = ((g64[:, None] - g64[None]) ** 2).sum(-1).astype(F32)
    assert not np.array_equal(bits(plain), bits(d))


def test_descriptor_longer_than_one_lds_chunk():
    """dim = 2500: the queries' descriptors pass through LDS in three pieces"""
    g = cases.clustered(40, 2500, seed=8)
    d = ref.distance_matrix(g)
    index, dist = ref.knn_lists(d, 39)
    check(g, 5, d, index, dist)


# ------------------------------------------------------------------------------------------------ 2. the independent route
@pytest.mark.parametrize("n, dim, k", [(65, 128, 20), (257, 33, 20), (1500, 128, 20), (6200, 3, 5)],
                         ids=["65", "257", "1500", "6200"])
def test_independent_route_on_exact_distances(n, dim, k):
    """small-integer descriptors: every distance is exact in any order, so float64 numpy and a (distance, index) sort give the
    kNN lists, and the closed form on those lists the pairs.  1 500 images: a row is six passes of a workgroup's lanes.
    6 200 images: 775 groups of 8 queries, more than the kernel launches workgroups, so that some take a second group."""
    g = cases.tied_integers(n, dim, seed=n)
    index, dist = cases.f64_knn(g, k)
    pairs, stats, knn_index, knn_distance = matching.graph_match(g, k, want_knn=True)
    assert np.array_equal(knn_index, index)
    assert np.array_equal(bits(knn_distance), bits(dist))
    rows, num_ranked = ref.graph_match_rows(index)
    assert np.array_equal(pairs, np.asarray(rows, np.int32))
    assert stats["num_pairs"] == len(rows) and stats["num_ranked_pairs"] == num_ranked
    if n >= 1500:
        assert len(rows) < n * (n - 1) // 4                           # a selection, far from everything


def test_whole_long_row_sorted():
    """4 100 images, k = 2 100: k is no small part of the row, which is sorted whole where it lies.  Two lists of
    more than (N - 2) / 2 images out of the same N - 2 share one, so every pair is selected."""
    n, k = 4100, 2100
    g = cases.tied_integers(n, 3, seed=11)
    index, dist = cases.f64_knn(g, k)
    pairs, stats, knn_index, knn_distance = matching.graph_match(g, k, want_knn=True)
    assert np.array_equal(knn_index, index)
    assert np.array_equal(bits(knn_distance), bits(dist))
    assert np.array_equal(pairs, np.stack(np.triu_indices(n, 1), axis=1).astype(np.int32))
    assert stats["num_pairs"] == n * (n - 1) // 2 and stats["num_nearest_neighbors"] == k


# ------------------------------------------------------------------------------------------------ 3. pooling
COUNTS = [1, 2, 63, 64, 65, 1000]


@pytest.mark.parametrize("dim", [1, 3, 128, 130])
def test_pooling_bit_for_bit(dim):
    rng = np.random.default_rng(dim)
    descs = [(rng.standard_normal((c, dim)) * 10.0 ** rng.integers(-3, 4, size=(c, 1))).astype(F32) for c in COUNTS]
    got = matching.mean_pool_descriptors(descs)
    assert got.dtype == F32 and got.shape == (len(COUNTS), dim)
    for i, d in enumerate(descs):
        assert np.array_equal(bits(got[i]), bits(ref.mean_pool(d))), COUNTS[i]
    assert np.array_equal(bits(matching.FisherVectorExtractor().ExtractGlobalDescriptor(descs[3])), bits(got[3]))


def test_pooling_rows_do_not_leak():
    rng = np.random.default_rng(5)
    small = [rng.standard_normal((c, 3)).astype(F32) for c in (1, 64, 65)]
    huge = lambda c: np.full((c, 3), 1e30, F32)
    descs = [huge(2), small[0], huge(1), small[1], huge(64), small[2], huge(3)]
    got = matching.mean_pool_descriptors(descs)
    for i, d in enumerate(descs):
        assert np.array_equal(bits(got[i]), bits(ref.mean_pool(d))), i
    assert np.abs(got[1::2]).max() < 10.0


def test_pooling_refuses_a_nan():
    descs = [np.ones((5, 4), F32), np.ones((70, 4), F32)]
    descs[1][69, 3] = np.nan
    feat_off = np.array([0, 5, 75], np.int64)
    flat = np.ascontiguousarray(np.concatenate(descs))
    out = np.full((2, 4), -7, F32)
    rc = capi.lib().theia_hip_mean_pool_descriptors(2, capi.ptr(feat_off, C.c_int64), 4, capi.ptr(flat, C.c_float),
                                                    capi.ptr(out, C.c_float))
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT and (out == -7).all()
    with pytest.raises(capi.TheiaHipError):
        matching.mean_pool_descriptors(descs)
    descs[1][69, 3] = np.inf                                          # an infinity is a value: the reference checks hasNaN only
    assert matching.mean_pool_descriptors(descs)[1].tolist() == [1.0, 1.0, 1.0, np.inf]


# ------------------------------------------------------------------------------------------------ 4. capacity, determinism
def test_capacity_one_short_returns_the_count_and_leaves_the_arrays():
    g, d, _, _ = restated("clustered", 65, 32)
    want = ref.graph_match_sequential(d, 7)
    n = len(want)

    def call(capacity):
        p1 = np.full(n + 2, -7, np.int32); p2 = np.full(n + 2, -7, np.int32)
        count = C.c_int64(-7)
        rc = capi.lib().theia_hip_graph_match(65, 32, capi.ptr(np.ascontiguousarray(g), C.c_float), 7, capacity,
                                              capi.ptr(p1, C.c_int32), capi.ptr(p2, C.c_int32), C.byref(count), None, None, None)
        return rc, count.value, p1, p2

    rc, count, p1, p2 = call(n - 1)
    assert rc == 0 and count == n and (p1 == -7).all() and (p2 == -7).all()
    rc, count, p1, p2 = call(0)
    assert rc == 0 and count == n and (p1 == -7).all() and (p2 == -7).all()
    rc, count, p1, p2 = call(n)
    assert rc == 0 and count == n and (p1[n:] == -7).all() and (p2[n:] == -7).all()
    assert list(zip(p1[:n].tolist(), p2[:n].tolist())) == want


def test_two_calls_give_the_same_bytes():
    g = cases.clustered(1500, 32, seed=2)
    a = matching.graph_match(g, 20, want_knn=True)
    b = matching.graph_match(g, 20, want_knn=True)
    assert a[1] == b[1] and 0 < a[1]["num_expanded_pairs"] < a[1]["num_pairs"] < 1500 * 1499 // 2
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ 5. end to end
def _clustered_images(seed=6, clusters=3, per_cluster=4, nfeat=40, dim=32):
    """12 images in 3 clusters: the images of a cluster see the same features (descriptor noise 0.02), the clusters' features
    lie around different centres, so the pooled descriptors cluster as the images do."""
    rng = np.random.default_rng(seed)
    feats = []
    for c in range(clusters):
        base = (rng.standard_normal((nfeat, dim)) + 4.0 * rng.standard_normal(dim)).astype(F32)
        for _ in range(per_cluster):
            desc = (base + 0.02 * rng.standard_normal((nfeat, dim))).astype(F32)
            feats.append(matching.KeypointsAndDescriptors(rng.uniform(0, 500, (nfeat, 2)), desc[rng.permutation(nfeat)]))
    return [f"img{i:02d}.jpg" for i in range(len(feats))], feats


def _matcher(names, feats):
    o = matching.FeatureMatcherOptions()
    o.perform_geometric_verification = False
    o.min_num_feature_matches = 10
    m = matching.BruteForceFeatureMatcher(o)
    m.AddImages(names, feats)
    return m


def _summary(out):
    return [(r.image1, r.image2, np.array([c.feature1 for c in r.correspondences]).tobytes(),
             np.array([c.feature2 for c in r.correspondences]).tobytes()) for r in out]


def test_selection_feeds_the_matcher(monkeypatch):
    names, feats = _clustered_images()
    seen = []
    inner = matching.brute_force_match_pairs

    def recording(descriptors_list, pairs, options):
        seen.append([tuple(p) for p in pairs])
        return inner(descriptors_list, pairs, options)

    monkeypatch.setattr(matching, "brute_force_match_pairs", recording)
    everything = _matcher(names, feats).MatchImages()
    assert len(seen[-1]) == 66 and len(everything) == 18              # only the pairs inside a cluster match

    m = _matcher(names, feats)
    selected = matching.SelectImagePairsWithGlobalDescriptorMatching(m, 2)
    pooled = np.stack([ref.mean_pool(f.descriptors) for f in feats])
    want = [(names[a], names[b]) for a, b in ref.graph_match(pooled, 2)[0]]
    assert selected == sorted(want) == m.pairs_to_match_
    assert all(names.index(a) // 4 == names.index(b) // 4 for a, b in selected) and len(selected) < 66
    out = m.MatchImages()
    assert seen[-1] == [(names.index(a), names.index(b)) for a, b in selected]    # the matcher touched those pairs and no other
    assert [(r.image1, r.image2) for r in out] == selected
    assert _summary(out) == [s for s in _summary(everything) if (s[0], s[1]) in set(selected)]

    # k >= N - 1 selects every pair: the default all-pairs call
    for k in (11, 100):
        m = _matcher(names, feats)
        assert len(matching.SelectImagePairsWithGlobalDescriptorMatching(m, k)) == 66
        assert _summary(m.MatchImages()) == _summary(everything)
