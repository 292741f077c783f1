"""Host-side mirror of pyTheia's matching interface (src/pytheia/matching/matching.cc:62-102) around the brute-force feature
matcher: FeatureMatcher::MatchImages (matching/feature_matcher.cc:104-228) with BruteForceFeatureMatcher::MatchImagePair
(matching/brute_force_feature_matcher.cc:48-115).  Every pair of the match graph goes through ONE
theia_hip_brute_force_match_pairs call (csrc/brute_force_matcher.hip: the distance matrices on the FP32 MFMA, the pair rule on
the device); the pairs that matched then go through twoview.VerifyMatchesIndexedBatch as one batch.

Stated deviations: AddImage takes the features (and the optional intrinsics prior) itself, the role of the reference's
FeaturesAndMatchesDatabase; MatchImages returns the ImagePairMatch list in pairs_to_match order (the reference's database fills
in the order its thread pool finishes); num_threads is kept for the interface only."""
import ctypes as C

import numpy as np

from . import _capi as capi
from . import twoview as _tv
from .twoview import KeypointsAndDescriptors, TwoViewInfo  # noqa: F401  (pyTheia's names)


class FeatureMatcherOptions:  # feature_matcher_options.h:43-88 (the fields pyTheia binds)
    def __init__(self):
        self.num_threads = 1
        self.keep_only_symmetric_matches = True
        self.use_lowes_ratio = True
        self.lowes_ratio = 0.8
        self.perform_geometric_verification = True
        self.geometric_verification_options = _tv.TwoViewMatchGeometricVerificationOptions()
        self.min_num_feature_matches = 30
        self.max_pairs_per_launch = 0   # this library's: 0 = chunks sized to the workspace budget; the result does not depend on it

    def to_c(self):
        o = capi.BruteForceOptions()
        capi.lib().theia_hip_brute_force_options_default(C.byref(o))
        o.keep_only_symmetric_matches = int(bool(self.keep_only_symmetric_matches))
        o.use_lowes_ratio = int(bool(self.use_lowes_ratio))
        o.lowes_ratio = float(self.lowes_ratio)
        o.min_num_feature_matches = int(self.min_num_feature_matches)
        o.max_pairs_per_launch = int(self.max_pairs_per_launch)
        return o


class IndexedFeatureMatch:  # matching/indexed_feature_match.h
    def __init__(self, feature1_ind=-1, feature2_ind=-1, distance=0.0):
        self.feature1_ind = feature1_ind
        self.feature2_ind = feature2_ind
        self.distance = distance

    def __eq__(self, other):
        return (self.feature1_ind, self.feature2_ind, self.distance) == (other.feature1_ind, other.feature2_ind, other.distance)

    def __repr__(self):
        return f"IndexedFeatureMatch({self.feature1_ind}, {self.feature2_ind}, {self.distance!r})"


class FeatureCorrespondence:  # matching/feature_correspondence.h
    def __init__(self, feature1=(0.0, 0.0), feature2=(0.0, 0.0)):
        self.feature1 = np.asarray(feature1, dtype=np.float64)
        self.feature2 = np.asarray(feature2, dtype=np.float64)


class ImagePairMatch:  # matching/image_pair_match.h
    def __init__(self):
        self.image1 = ""
        self.image2 = ""
        self.twoview_info = TwoViewInfo()
        self.correspondences = []


def brute_force_knn2(desc1, desc2):
    """theia_hip_brute_force_knn2: (fwd_dist [n1][2], fwd_index, rev_dist [n2][2], rev_index), the search without the pair rule."""
    desc1 = np.ascontiguousarray(desc1, dtype=np.float32); desc2 = np.ascontiguousarray(desc2, dtype=np.float32)
    n1, n2, dim = len(desc1), len(desc2), desc1.shape[1]
    if desc2.shape[1] != dim:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "descriptor lengths differ")
    fd = np.zeros((n1, 2), np.float32); fi = np.zeros((n1, 2), np.int32)
    rd = np.zeros((n2, 2), np.float32); ri = np.zeros((n2, 2), np.int32)
    capi.check(capi.lib().theia_hip_brute_force_knn2(n1, n2, dim, capi.ptr(desc1, C.c_float), capi.ptr(desc2, C.c_float),
                                                      capi.ptr(fd, C.c_float), capi.ptr(fi, C.c_int32), capi.ptr(rd, C.c_float),
                                                      capi.ptr(ri, C.c_int32)))
    return fd, fi, rd, ri


def brute_force_match_pairs(descriptors_list, pairs, options):
    """theia_hip_brute_force_match_pairs on a list of per-image descriptor arrays [n_i][dim] and (image1, image2) index pairs:
    (pair_ok [num_pairs] bool, match_off [num_pairs + 1], feature1, feature2, distance)."""
    descs = [np.ascontiguousarray(d, dtype=np.float32) for d in descriptors_list]
    dims = {d.shape[1] for d in descs if d.ndim == 2 and len(d)}
    if len(dims) > 1:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "descriptor lengths differ")
    dim = dims.pop() if dims else 1
    feat_off = np.zeros(len(descs) + 1, dtype=np.int64)
    feat_off[1:] = np.cumsum([len(d) for d in descs])
    flat = np.ascontiguousarray(np.concatenate([d.reshape(-1, dim) for d in descs]) if descs else np.zeros((0, dim), np.float32))
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    p1 = np.ascontiguousarray(pairs[:, 0]); p2 = np.ascontiguousarray(pairs[:, 1])
    inside = (p1 >= 0) & (p1 < len(descs))
    capacity = int(sum(len(descs[i]) for i in p1[inside]))
    ok = np.zeros(len(pairs), np.uint8); off = np.zeros(len(pairs) + 1, np.int64)
    f1 = np.zeros(capacity, np.int32); f2 = np.zeros(capacity, np.int32); dist = np.zeros(capacity, np.float32)
    o = options.to_c() if hasattr(options, "to_c") else options
    capi.check(capi.lib().theia_hip_brute_force_match_pairs(
        len(descs), capi.ptr(feat_off, C.c_int64), dim, capi.ptr(flat, C.c_float), len(pairs), capi.ptr(p1, C.c_int32),
        capi.ptr(p2, C.c_int32), C.byref(o), capi.ptr(ok, C.c_uint8), capi.ptr(off, C.c_int64), capi.ptr(f1, C.c_int32),
        capi.ptr(f2, C.c_int32), capi.ptr(dist, C.c_float)))
    n = int(off[-1])
    return ok.astype(bool), off, f1[:n], f2[:n], dist[:n]


class BruteForceFeatureMatcher:
    """FeatureMatcher with MatchImagePair = BruteForceFeatureMatcher's (feature_matcher.h:77-160)."""

    def __init__(self, options=None):
        self.options_ = options if options is not None else FeatureMatcherOptions()
        self.image_names_ = []
        self.features_ = {}
        self.intrinsics_ = {}
        self.pairs_to_match_ = []

    def AddImage(self, image_name, features, intrinsics_prior=None):
        self.image_names_.append(image_name)
        self.features_[image_name] = features
        if intrinsics_prior is not None:
            self.intrinsics_[image_name] = intrinsics_prior

    def AddImages(self, image_names, features_list, intrinsics_priors=None):
        for k, name in enumerate(image_names):
            self.AddImage(name, features_list[k], None if intrinsics_priors is None else intrinsics_priors[k])

    def SetImagePairsToMatch(self, pairs_to_match):
        self.pairs_to_match_ = [tuple(p) for p in pairs_to_match]

    def MatchImagePair(self, features1, features2):
        """(ok, [IndexedFeatureMatch]) of one pair."""
        ok, off, f1, f2, dist = brute_force_match_pairs([features1.descriptors, features2.descriptors], [(0, 1)], self.options_)
        return bool(ok[0]), [IndexedFeatureMatch(int(a), int(b), d) for a, b, d in zip(f1, f2, dist)]

    def MatchImages(self):
        """All pairs i < j if none were set (feature_matcher.cc:63-77, :104-109); returns [ImagePairMatch] of the pairs that matched
        (and, with perform_geometric_verification, verified), in pairs_to_match order."""
        if not self.pairs_to_match_:
            names = self.image_names_
            self.pairs_to_match_ = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
        index = {name: k for k, name in enumerate(self.image_names_)}
        feats = [self.features_[name] for name in self.image_names_]
        pairs = [(index[a], index[b]) for a, b in self.pairs_to_match_]
        ok, off, f1, f2, _ = brute_force_match_pairs([f.descriptors for f in feats], pairs, self.options_)
        live = [k for k in range(len(pairs)) if ok[k]]
        putative = {k: np.stack([f1[off[k]:off[k + 1]], f2[off[k]:off[k + 1]]], axis=1).astype(np.int64) for k in live}
        out = []
        if self.options_.perform_geometric_verification:
            prior = lambda name: self.intrinsics_.get(name, _tv.CameraIntrinsicsPrior())   # feature_matcher.cc:203-215
            res = _tv.VerifyMatchesIndexedBatch(self.options_.geometric_verification_options,
                                                [prior(self.pairs_to_match_[k][0]) for k in live],
                                                [prior(self.pairs_to_match_[k][1]) for k in live],
                                                [feats[pairs[k][0]] for k in live], [feats[pairs[k][1]] for k in live],
                                                [putative[k] for k in live]) if live else []
            verified = {k: r for k, r in zip(live, res)}
        for k in live:
            fa, fb = feats[pairs[k][0]], feats[pairs[k][1]]
            m = ImagePairMatch()
            m.image1, m.image2 = self.pairs_to_match_[k]
            if self.options_.perform_geometric_verification:
                good, info, idx = verified[k]
                if not good:
                    continue
                m.twoview_info = info
            else:
                idx = putative[k]
            m.correspondences = [FeatureCorrespondence(fa.keypoints[a], fb.keypoints[b]) for a, b in idx]
            out.append(m)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# Image-pair selection by global descriptors (csrc/graph_match.hip): FisherVectorExtractor (matching/
# fisher_vector_extractor.cc:56-69, the element-wise mean in the reference's fork), GraphMatch (matching/graph_match.cc:48-130)
# and FeatureExtractorAndMatcher::SelectImagePairsWithGlobalDescriptorMatching (sfm/feature_extractor_and_matcher.cc:356-381).


def mean_pool_descriptors(descriptors_list):
    """theia_hip_mean_pool_descriptors on a list of per-image descriptor arrays [n_i][dim]: the global descriptors
    [num_images][dim], float32."""
    descs = [np.ascontiguousarray(d, dtype=np.float32) for d in descriptors_list]
    descs = [d.reshape(len(d), -1) if d.ndim != 2 else d for d in descs]
    dims = {d.shape[1] for d in descs if len(d)}
    if len(dims) > 1:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "descriptor lengths differ")
    dim = dims.pop() if dims else 1
    feat_off = np.zeros(len(descs) + 1, dtype=np.int64)
    feat_off[1:] = np.cumsum([len(d) for d in descs])
    flat = np.ascontiguousarray(np.concatenate([d.reshape(-1, dim) for d in descs]) if descs else np.zeros((0, dim), np.float32))
    out = np.zeros((len(descs), dim), np.float32)
    capi.check(capi.lib().theia_hip_mean_pool_descriptors(len(descs), capi.ptr(feat_off, C.c_int64), dim, capi.ptr(flat, C.c_float),
                                                           capi.ptr(out, C.c_float)))
    return out


def graph_match(global_descriptors, k, want_knn=False):
    """theia_hip_graph_match on global descriptors [num_images][dim]: (pairs [num_pairs][2] int32 with image1 < image2, ascending,
    stats dict), and with want_knn also (knn_index [num_images][k'], knn_distance [num_images][k']), k' = min(num_images - 1, k)."""
    g = np.ascontiguousarray(global_descriptors, dtype=np.float32)
    if g.ndim != 2:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "global descriptors must be [num_images][dim]")
    n, dim = g.shape
    k = int(k)
    L = capi.lib()
    count = C.c_int64(0)
    stats = capi.GraphMatchStats()
    kk = max(0, min(n - 1, k))
    knn_index = np.zeros((n, kk), np.int32) if want_knn else None
    knn_distance = np.zeros((n, kk), np.float32) if want_knn else None

    def call(capacity, p1, p2):
        capi.check(L.theia_hip_graph_match(n, dim, capi.ptr(g, C.c_float), k, capacity, capi.ptr(p1, C.c_int32),
                                           capi.ptr(p2, C.c_int32), C.byref(count), capi.ptr(knn_index, C.c_int32),
                                           capi.ptr(knn_distance, C.c_float), C.byref(stats)))

    # a row holds about 2 k^2 + k pairs where the inverse lists are about as long as the lists (and there are never more than all
    # pairs): one call where that guess is a modest array, else the count first; a count beyond the guess repeats the call
    guess = min(n * (n - 1) // 2, n * (2 * kk * kk + kk))
    capacity = guess if guess <= (1 << 24) else 0
    p1 = np.zeros(capacity, np.int32); p2 = np.zeros(capacity, np.int32)
    call(capacity, p1, p2)
    if count.value > capacity:
        capacity = count.value
        p1 = np.zeros(capacity, np.int32); p2 = np.zeros(capacity, np.int32)
        call(capacity, p1, p2)
    pairs = np.stack([p1[:count.value], p2[:count.value]], axis=1)
    if want_knn:
        return pairs, stats.as_dict(), knn_index, knn_distance
    return pairs, stats.as_dict()


class FisherVectorExtractor:
    """matching/fisher_vector_extractor.h in the reference's shape: the options and the training calls are kept and do nothing,
    ExtractGlobalDescriptor is the element-wise mean of the features."""

    class Options:
        def __init__(self):
            self.num_gmm_clusters = 16
            self.max_num_features_for_training = 100000

    def __init__(self, options=None):
        self.options_ = options if options is not None else FisherVectorExtractor.Options()

    def AddFeaturesForTraining(self, features):
        pass

    def Train(self):
        return True

    def ExtractGlobalDescriptor(self, features):
        return mean_pool_descriptors([np.asarray(features, dtype=np.float32)])[0]


def GraphMatch(image_names, global_descriptors, num_nearest_neighbors_for_global_descriptor_matching):
    """[(name, name)]: every selected pair oriented by image index, the list sorted by the pair of names (graph_match.cc:125-128)."""
    names = list(image_names)
    g = np.asarray(global_descriptors, dtype=np.float32).reshape(len(names), -1) if len(names) else np.zeros((0, 1), np.float32)
    pairs, _ = graph_match(g, num_nearest_neighbors_for_global_descriptor_matching)
    return sorted((names[a], names[b]) for a, b in pairs.tolist())


def SelectImagePairsWithGlobalDescriptorMatching(matcher, num_nearest_neighbors=100):
    """Pools the features of matcher.image_names_ in AddImage order (stated deviation: the reference takes the order of its
    database's ImageNamesOfFeatures), runs GraphMatch and hands the pairs to matcher.SetImagePairsToMatch; returns them."""
    names = list(matcher.image_names_)
    if not FisherVectorExtractor().Train():
        raise RuntimeError("the global descriptor extractor did not train")
    pooled = mean_pool_descriptors([matcher.features_[name].descriptors for name in names])
    pairs = GraphMatch(names, pooled, num_nearest_neighbors)
    matcher.SetImagePairsToMatch(pairs)
    return pairs
