"""GPU: the brute-force feature matcher (csrc/brute_force_matcher.hip: BruteForceFeatureMatcher::MatchImagePair,
matching/brute_force_feature_matcher.cc:48-115, for a whole match graph) against the sequential numpy restatement in
tests/brute_force_matcher_ref.py -- distances bit for bit (the FP32 MFMA is a k-ordered fmaf chain), the pair rule array for
array, and the pyTheia-named mirror in pytheiasfm_amd/matching.py."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, matching, synth, twoview as tv
from tests import brute_force_matcher_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. the search alone
@pytest.mark.parametrize("dim", [1, 3, 32, 36, 100, 128, 130])
@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 1), (1, 2), (31, 33), (127, 129), (130, 300), (300, 130)])
def test_knn2_bit_for_bit(n1, n2, dim):
    """Shapes on both sides of the 128-tile and of the 32-chunk of K, an odd K (zero padded to the MFMA's k pair), both load
    paths of the tile kernel with a short last chunk (dim 36 and 100: float4 loads; 1, 3 and 130: scalar loads), a row of zeros,
    and planted ties across two column blocks / two row blocks: candidates 5 and 200 hold the same descriptor, a query equal to it
    sees both at distance 0 and must list 5 first."""
    rng = np.random.default_rng(1000 * n1 + 10 * n2 + dim)
    d1 = (3.0 * rng.standard_normal((n1, dim))).astype(F32); d2 = (3.0 * rng.standard_normal((n2, dim))).astype(F32)
    if n1 >= 2:
        d1[n1 // 2] = 0
    if n2 >= 2:
        d2[n2 // 2] = 0
    if n2 > 200:
        d2[200] = d2[5]; d1[7] = d2[5]
    if n1 > 200:
        d1[200] = d1[5]; d2[9] = d1[5]
    fd, fi, rd, ri = matching.brute_force_knn2(d1, d2)
    wfd, wfi, wrd, wri = ref.knn2(d1, d2)
    # the float64 running-error bound of the chain, on the direct form: (dim + 4) 2^-24 (|a|^2 + |b|^2 + 2 sum |a_k b_k|)
    a = d1.astype(np.float64); b = d2.astype(np.float64)
    d64 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    bound = (dim + 4) * 2.0 ** -24 * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2 * np.abs(a) @ np.abs(b).T)
    worst = 0.0
    for dist, index, mat, bnd in ((fd, fi, d64, bound), (rd, ri, d64.T, bound.T)):
        for i in range(len(dist)):
            for s in range(2):
                if index[i, s] >= 0:
                    e = abs(float(dist[i, s]) - mat[i, index[i, s]])
                    assert e <= bnd[i, index[i, s]], (i, s, e, bnd[i, index[i, s]])
                    worst = max(worst, e / max(bnd[i, index[i, s]], 1e-300))
    print(f"knn2 {n1} x {n2} x {dim}: largest error / bound = {worst:.4f}")
    assert np.array_equal(fi, wfi) and np.array_equal(ri, wri)
    assert np.array_equal(fd.view(np.uint32), wfd.view(np.uint32)) and np.array_equal(rd.view(np.uint32), wrd.view(np.uint32))
    if n2 > 200:
        assert fi[7].tolist() == [5, 200] and fd[7].tolist() == [0, 0]
    if n1 > 200:
        assert ri[9].tolist() == [5, 200] and rd[9].tolist() == [0, 0]
    if n2 == 1:
        assert (fi[:, 1] == -1).all() and np.isinf(fd[:, 1]).all()
    if n1 == 1:
        assert (ri[:, 1] == -1).all() and np.isinf(rd[:, 1]).all()


# ------------------------------------------------------------------------------------------------ 2. - 4. the match graph
SIZES = [0, 1, 40, 129, 257, 300]


@pytest.fixture(scope="module")
def graph():
    """Six images that see subsets of 300 common descriptors (dim 32) plus noise; all 15 pairs, one pair listed twice, one self
    pair.  The restatement's searches are computed once and shared."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((300, 32)).astype(F32)
    descs = []
    for n in SIZES:
        rows = rng.permutation(300)[:n]
        descs.append((base[rows] + 0.25 * rng.standard_normal((n, 32))).astype(F32))
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(3, 4), (5, 5)]
    nn = {p: ref.knn2(descs[p[0]], descs[p[1]]) for p in set(pairs)}
    return descs, pairs, nn


def _options(symmetric, ratio_on, ratio, min_matches, per_launch=0):
    o = matching.FeatureMatcherOptions()
    o.keep_only_symmetric_matches = symmetric; o.use_lowes_ratio = ratio_on; o.lowes_ratio = ratio
    o.min_num_feature_matches = min_matches; o.max_pairs_per_launch = per_launch
    return o


@pytest.mark.parametrize("min_matches", [0, 30])
@pytest.mark.parametrize("ratio", [0.6, 0.8])
@pytest.mark.parametrize("symmetric,ratio_on", [(True, True), (True, False), (False, True), (False, False)])
def test_match_pairs_equals_the_restatement(graph, symmetric, ratio_on, ratio, min_matches):
    descs, pairs, nn = graph
    ok, off, f1, f2, dist = matching.brute_force_match_pairs(descs, pairs, _options(symmetric, ratio_on, ratio, min_matches))
    assert off[0] == 0 and len(off) == len(pairs) + 1
    some = 0
    for k, p in enumerate(pairs):
        wok, want = ref.pair_rule(nn[p], keep_only_symmetric_matches=symmetric, use_lowes_ratio=ratio_on, lowes_ratio=ratio,
                                  min_num_feature_matches=min_matches)
        assert bool(ok[k]) == wok, (k, p)
        s = slice(int(off[k]), int(off[k + 1]))
        assert f1[s].tolist() == [m[0] for m in want] and f2[s].tolist() == [m[1] for m in want], (k, p)
        assert np.array_equal(dist[s].view(np.uint32), np.array([m[2] for m in want], F32).view(np.uint32)), (k, p)
        some += len(want)
    assert some > 300                                    # the graph is not empty under any of the settings
    assert not ok[0] or min_matches == 0                 # image 0 has no features: no matches, ok only when none are asked for


def test_chunking_changes_nothing(graph):
    descs, pairs, _ = graph
    outs = [matching.brute_force_match_pairs(descs, pairs, _options(True, True, 0.8, 30, per_launch=n)) for n in (0, 1, 3)]
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_invalid_arguments_leave_the_outputs_untouched(graph):
    descs, pairs, _ = graph
    L = capi.lib()
    P = capi.ptr
    flat = np.ascontiguousarray(np.concatenate(descs))
    feat_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    p1 = np.array([p[0] for p in pairs], np.int32); p2 = np.array([p[1] for p in pairs], np.int32)
    cap = int(sum(SIZES[i] for i in p1))
    o = matching.FeatureMatcherOptions().to_c()

    def call(num_images=6, off=feat_off, dim=32, desc=flat, num_pairs=len(pairs), a=p1, b=p2, opts=o, null=()):
        ok = np.full(len(pairs), 7, np.uint8); moff = np.full(len(pairs) + 1, -5, np.int64)
        f1 = np.full(cap, -5, np.int32); f2 = np.full(cap, -5, np.int32); dist = np.full(cap, -5.0, F32)
        outs = {"ok": ok, "off": moff, "f1": f1, "f2": f2, "dist": dist}
        arg = lambda name, t: P(None if name in null else outs[name], t)
        rc = L.theia_hip_brute_force_match_pairs(num_images, P(off, C.c_int64), dim, P(desc, C.c_float), num_pairs, P(a, C.c_int32),
                                                 P(b, C.c_int32), C.byref(opts) if opts is not None else None, arg("ok", C.c_uint8),
                                                 arg("off", C.c_int64), arg("f1", C.c_int32), arg("f2", C.c_int32), arg("dist", C.c_float))
        return rc, outs

    def refused(**kw):
        rc, outs = call(**kw)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, kw.keys()
        assert (outs["ok"] == 7).all() and (outs["off"] == -5).all() and (outs["f1"] == -5).all() and (outs["f2"] == -5).all()
        assert (outs["dist"] == -5.0).all()

    refused(dim=0)
    refused(num_images=-1)
    refused(num_pairs=-1)
    refused(desc=None)
    refused(off=None)
    refused(a=None)
    refused(opts=None)
    for name in ("ok", "off", "f1", "f2", "dist"):
        refused(null=(name,))
    bad = p1.copy(); bad[3] = 6
    refused(a=bad)
    bad = p2.copy(); bad[0] = -1
    refused(b=bad)
    dec = feat_off.copy(); dec[3] = dec[2] - 1
    refused(off=dec)
    rc, outs = call(num_pairs=0)                          # zero pairs: valid, match_off = [0]
    assert rc == 0 and outs["off"][0] == 0 and (outs["off"][1:] == -5).all() and (outs["ok"] == 7).all()
    rc, outs = call()
    assert rc == 0 and outs["off"][0] == 0 and (np.diff(outs["off"]) >= 0).all()
    # the search alone
    out = [np.zeros((4, 2), F32), np.zeros((4, 2), np.int32), np.zeros((4, 2), F32), np.zeros((4, 2), np.int32)]
    d = np.ones((4, 8), F32)
    args = lambda n1, n2, dim, x: (n1, n2, dim, P(x, C.c_float), P(d, C.c_float), P(out[0], C.c_float), P(out[1], C.c_int32),
                                   P(out[2], C.c_float), P(out[3], C.c_int32))
    assert L.theia_hip_brute_force_knn2(*args(4, 4, 0, d)) == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert L.theia_hip_brute_force_knn2(*args(-1, 4, 8, d)) == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert L.theia_hip_brute_force_knn2(*args(4, 4, 8, None)) == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert all((x == 0).all() for x in out)


def test_non_finite_descriptors_are_refused(graph):
    """A NaN or infinite descriptor value (or values whose squared norm overflows float) makes every distance to that feature NaN:
    THEIA_HIP_ERR_INVALID_ARGUMENT from both entry points, outputs untouched."""
    descs, pairs, _ = graph
    for value, where in ((np.nan, (3, 17, 5)), (np.inf, (5, 299, 31)), (-np.inf, (2, 0, 0)), (3e19, (4, 100, 7))):
        bad = [d.copy() for d in descs]
        bad[where[0]][where[1], where[2]] = value
        flat = np.ascontiguousarray(np.concatenate(bad))
        feat_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
        p1 = np.array([p[0] for p in pairs], np.int32); p2 = np.array([p[1] for p in pairs], np.int32)
        cap = int(sum(SIZES[i] for i in p1))
        ok = np.full(len(pairs), 7, np.uint8); off = np.full(len(pairs) + 1, -5, np.int64)
        f1 = np.full(cap, -5, np.int32); f2 = np.full(cap, -5, np.int32); dist = np.full(cap, -5.0, F32)
        o = matching.FeatureMatcherOptions().to_c()
        P = capi.ptr
        rc = capi.lib().theia_hip_brute_force_match_pairs(6, P(feat_off, C.c_int64), 32, P(flat, C.c_float), len(pairs), P(p1, C.c_int32),
                                                          P(p2, C.c_int32), C.byref(o), P(ok, C.c_uint8), P(off, C.c_int64),
                                                          P(f1, C.c_int32), P(f2, C.c_int32), P(dist, C.c_float))
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, value
        assert (ok == 7).all() and (off == -5).all() and (f1 == -5).all() and (f2 == -5).all() and (dist == -5.0).all()
        with pytest.raises(capi.TheiaHipError):
            matching.brute_force_knn2(bad[where[0]], descs[3])
        with pytest.raises(capi.TheiaHipError):
            matching.brute_force_knn2(descs[3], bad[where[0]])
    assert matching.brute_force_match_pairs(descs, pairs, matching.FeatureMatcherOptions())[1][0] == 0   # and the clean graph still runs


# ------------------------------------------------------------------------------------------------ 5. the mirror
def _three_views(seed=4, npts=300, nextra=80, dim=32):
    """Three pinhole views (f = 800, 1000 x 800 px) of npts points: every visible point is a feature of all three images with
    (nearly) the same descriptor, nextra distractors per image, the feature indices of images 1 and 2 permuted."""
    rng = np.random.default_rng(seed)
    intr = np.array([800.0, 1.0, 0.0, 500.0, 400.0, 0.0, 0.0])
    exts = [np.zeros(6), np.array([1.0, 0.1, 0.05, 0.02, -0.15, 0.03]), np.array([-0.9, 0.05, 0.1, -0.03, 0.12, 0.02])]
    X = np.concatenate([rng.uniform(-2.5, 2.5, (npts, 2)), rng.uniform(5.0, 9.0, (npts, 1)), np.ones((npts, 1))], axis=1)
    uvs, vis = [], np.ones(npts, bool)
    for e in exts:
        uv, ok = synth.project(0, np.tile(intr, (npts, 1)), np.tile(e, (npts, 1)), X)
        vis &= ok & (uv > 0).all(1) & (uv[:, 0] < 1000) & (uv[:, 1] < 800)
        uvs.append(uv)
    n = int(vis.sum())
    base = rng.standard_normal((n, dim)).astype(F32)
    feats, truth = [], []
    for v in range(3):
        k = np.concatenate([uvs[v][vis] + 0.3 * rng.standard_normal((n, 2)), rng.uniform([5, 5], [995, 795], (nextra, 2))])
        d = np.concatenate([base + 0.05 * rng.standard_normal((n, dim)).astype(F32), rng.standard_normal((nextra, dim)).astype(F32)])
        perm = np.arange(len(k)) if v == 0 else rng.permutation(len(k))
        feats.append(tv.KeypointsAndDescriptors(k[perm], d[perm]))
        truth.append(np.argsort(perm)[:n])                 # point -> feature index in this image
    prior = tv.CameraIntrinsicsPrior(); prior.image_width = 1000; prior.image_height = 800
    prior.focal_length.is_set = True; prior.focal_length.value = [800.0]
    prior.principal_point.is_set = True; prior.principal_point.value = [500.0, 400.0]
    return feats, truth, prior


def test_mirror_follows_the_restatement_and_the_verification():
    feats, truth, prior = _three_views()
    names = ["a.jpg", "b.jpg", "c.jpg"]
    o = matching.FeatureMatcherOptions()
    o.geometric_verification_options.estimate_twoview_info_options.seed = 9
    o.geometric_verification_options.estimate_twoview_info_options.max_sampson_error_pixels = 2.0
    m = matching.BruteForceFeatureMatcher(o)
    m.AddImages(names, feats, [prior] * 3)
    pairs = [(0, 1), (0, 2), (1, 2)]
    putative = {}
    for i, j in pairs:
        ok, got = m.MatchImagePair(feats[i], feats[j])
        wok, want = ref.match_image_pair(feats[i].descriptors, feats[j].descriptors)
        assert ok and wok
        assert [(g.feature1_ind, g.feature2_ind) for g in got] == [(w[0], w[1]) for w in want]
        assert [np.float32(g.distance).view(np.uint32) for g in got] == [np.float32(w[2]).view(np.uint32) for w in want]
        right = {int(a): int(b) for a, b in zip(truth[i], truth[j])}
        assert all(right.get(g.feature1_ind) == g.feature2_ind for g in got)          # none wrong on this margin scene
        assert len(got) > 0.95 * len(right)
        putative[(i, j)] = [(w[0], w[1]) for w in want]
    # with verification: restatement matches -> VerifyMatchesIndexedBatch, pair for pair, in pairs_to_match order
    out = m.MatchImages()
    want = tv.VerifyMatchesIndexedBatch(o.geometric_verification_options, [prior] * 3, [prior] * 3, [feats[i] for i, _ in pairs],
                                        [feats[j] for _, j in pairs], [putative[p] for p in pairs])
    assert m.pairs_to_match_ == [(names[i], names[j]) for i, j in pairs]
    assert [(r.image1, r.image2) for r in out] == [(names[i], names[j]) for (i, j), w in zip(pairs, want) if w[0]] and len(out) == 3
    for r, (i, j), (ok, info, idx) in zip(out, pairs, want):
        assert len(r.correspondences) == len(idx) == r.twoview_info.num_verified_matches > 100
        assert np.array_equal(np.array([c.feature1 for c in r.correspondences]), feats[i].keypoints[[a for a, _ in idx]])
        assert np.array_equal(np.array([c.feature2 for c in r.correspondences]), feats[j].keypoints[[b for _, b in idx]])
        assert np.array_equal(r.twoview_info.rotation_2, info.rotation_2) and np.array_equal(r.twoview_info.position_2, info.position_2)
        assert r.twoview_info.num_homography_inliers == info.num_homography_inliers
    # without verification: the keypoint pairs of the putative matches; an explicit pair list keeps its order
    o.perform_geometric_verification = False
    m.SetImagePairsToMatch([(names[1], names[2]), (names[0], names[1])])
    out = m.MatchImages()
    assert [(r.image1, r.image2) for r in out] == [(names[1], names[2]), (names[0], names[1])]
    for r, p in zip(out, [(1, 2), (0, 1)]):
        assert np.array_equal(np.array([c.feature1 for c in r.correspondences]), feats[p[0]].keypoints[[a for a, _ in putative[p]]])
        assert np.array_equal(np.array([c.feature2 for c in r.correspondences]), feats[p[1]].keypoints[[b for _, b in putative[p]]])
    # a pair below min_num_feature_matches is not returned
    o.min_num_feature_matches = 10 ** 6
    assert m.MatchImages() == []
