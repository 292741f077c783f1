"""Host-side mirror of pyTheia's TrackBuilder (pytheia.sfm, sfm.cc:941-942, :1020-1026; sfm/track_builder.cc) around
theia_hip_build_tracks (csrc/track_builder.hip): the matches of a whole match graph become tracks in ONE C-ABI call, the connected
components on the device.  The rule, the stated orders and the stated deviations are in include/theia_hip.h and DESIGN.md 3.6n.

build_tracks takes the indexed matches in the CSR form matching.brute_force_match_pairs and the indexed verification return.
TrackBuilder takes coordinates, as the reference's does: features of one view with equal (x, y) bit patterns are one node, and
BuildTracks numbers a view's features in the order of their first AddFeatureCorrespondence before the call (index_features), so
"the lowest feature index of a view" is the feature that view added first.  BuildTracksIncremental is not built."""
import ctypes as C

import numpy as np

from . import _capi as capi


class TrackBuilderOptions:  # reconstruction_builder.h:81-85
    def __init__(self, min_track_length=2, max_track_length=50):
        self.min_track_length = min_track_length
        self.max_track_length = max_track_length

    def to_c(self):
        o = capi.TrackBuilderOptions()
        o.min_track_length = int(self.min_track_length)
        o.max_track_length = int(self.max_track_length)
        return o


class Feature:  # sfm/feature.h: a point and its 2 x 2 covariance (identity unless given)
    def __init__(self, point=(0.0, 0.0), covariance=None):
        self.point_ = np.asarray(point, dtype=np.float64).reshape(2)
        self.covariance_ = np.eye(2) if covariance is None else np.asarray(covariance, dtype=np.float64).reshape(2, 2)


def _point_and_cov(feature):
    """A feature is a Feature, 2 coordinates, or (2 coordinates, covariance): (x, y, cov_xx, cov_yy)."""
    if isinstance(feature, Feature):
        return feature.point_[0], feature.point_[1], feature.covariance_[0, 0], feature.covariance_[1, 1]
    if len(feature) == 2 and np.ndim(feature[0]) == 1:
        cov = np.asarray(feature[1], dtype=np.float64).reshape(2, 2)
        return float(feature[0][0]), float(feature[0][1]), cov[0, 0], cov[1, 1]
    return float(feature[0]), float(feature[1]), 1.0, 1.0


def build_tracks(feat_off, pair_view1, pair_view2, match_off, feature1, feature2, options=None):
    """theia_hip_build_tracks: (track_off [num_tracks + 1], obs_view, obs_feature, obs_track, stats dict)."""
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    i8 = lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    feat_off, match_off = i8(feat_off), i8(match_off)
    pv1, pv2, f1, f2 = i4(pair_view1), i4(pair_view2), i4(feature1), i4(feature2)
    if len(feat_off) < 1 or len(match_off) != len(pv1) + 1 or len(pv2) != len(pv1) or len(f1) != len(f2):
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "array lengths do not fit")
    if match_off[-1] > len(f1):
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "match_off runs past the matches")
    if options is None:
        o = capi.TrackBuilderOptions()
        capi.lib().theia_hip_track_builder_options_default(C.byref(o))
    else:
        o = options.to_c() if hasattr(options, "to_c") else options
    m = max(int(match_off[-1]), 0)
    cap = max(0, min(2 * m, int(feat_off[-1])))
    track_off = np.zeros(m + 1, np.int64)
    obs_view = np.zeros(cap, np.int32); obs_feature = np.zeros(cap, np.int32); obs_track = np.zeros(cap, np.int32)
    st = capi.TrackBuilderStats()
    capi.check(capi.lib().theia_hip_build_tracks(
        len(feat_off) - 1, capi.ptr(feat_off, C.c_int64), len(pv1), capi.ptr(pv1, C.c_int32), capi.ptr(pv2, C.c_int32),
        capi.ptr(match_off, C.c_int64), capi.ptr(f1, C.c_int32), capi.ptr(f2, C.c_int32), C.byref(o),
        capi.ptr(track_off, C.c_int64), capi.ptr(obs_view, C.c_int32), capi.ptr(obs_feature, C.c_int32),
        capi.ptr(obs_track, C.c_int32), C.byref(st)))
    nt, no = int(st.num_tracks), int(st.num_observations)
    return track_off[:nt + 1], obs_view[:no], obs_feature[:no], obs_track[:no], st.as_dict()


def last_timings():
    """theia_hip_track_builder_last_timings of the calling thread, as a dict of milliseconds."""
    t = capi.TrackBuilderTimings()
    capi.check(capi.lib().theia_hip_track_builder_last_timings(C.byref(t)))
    return t.as_dict()


def index_features(views, xy, num_views=0):
    """The coordinate-to-index merge, on the host: rows (view, x, y) with equal bit patterns are one feature; a view's features
    are numbered in the order of their first row.  Returns (feat_off [nv + 1], feature index of every row, first row of every
    feature in node order), nv = max(num_views, largest view + 1)."""
    views = np.asarray(views, dtype=np.int64).reshape(-1)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    nv = max(int(num_views), int(views.max()) + 1 if len(views) else 0)
    if len(views) == 0:
        return np.zeros(nv + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)
    rows = np.column_stack([views, xy.view(np.int64)])
    uniq, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    order = np.lexsort((first, uniq[:, 0]))          # by view, then by first appearance
    node = np.empty(len(uniq), np.int64)
    node[order] = np.arange(len(uniq))
    feat_off = np.zeros(nv + 1, np.int64)
    feat_off[1:] = np.cumsum(np.bincount(uniq[:, 0], minlength=nv))
    node_of_row = node[inverse.reshape(-1)]
    return feat_off, (node_of_row - feat_off[views]).astype(np.int32), first[order]


class TrackBuilder:
    """theia::TrackBuilder (track_builder.h): AddFeatureCorrespondence collects, BuildTracks runs the whole graph in one call."""

    def __init__(self, min_track_length=2, max_track_length=50):
        self.options_ = TrackBuilderOptions(min_track_length, max_track_length)
        self.views_ = []      # [view1, view2] per correspondence
        self.rows_ = []       # [x1, y1, cxx1, cyy1, x2, y2, cxx2, cyy2]
        self.stats_ = None    # of the last BuildTracks

    def AddFeatureCorrespondence(self, view_id1, feature1, view_id2, feature2):
        if view_id1 == view_id2:   # track_builder.cc:66
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT,
                                     "cannot add 2 features from the same image as a correspondence")
        self.views_.append((int(view_id1), int(view_id2)))
        self.rows_.append(_point_and_cov(feature1) + _point_and_cov(feature2))

    def indexed(self, num_views=0):
        """The collected correspondences as build_tracks takes them: (feat_off, pair_view1, pair_view2, match_off, feature1,
        feature2, first), a run of correspondences between the same two views being one pair; first = per node the row of
        the interleaved (correspondence, side) list it first appeared in."""
        views = np.asarray(self.views_, dtype=np.int64).reshape(-1, 2)
        rows = np.asarray(self.rows_, dtype=np.float64).reshape(-1, 8)
        feat_off, feature, first = index_features(views.reshape(-1), rows.reshape(-1, 4)[:, :2], num_views)
        change = np.ones(len(views), bool)
        change[1:] = (views[1:] != views[:-1]).any(axis=1)
        start = np.nonzero(change)[0]
        match_off = np.append(start, len(views)).astype(np.int64)
        feature = feature.reshape(-1, 2)
        return (feat_off, views[start, 0].astype(np.int32), views[start, 1].astype(np.int32), match_off,
                np.ascontiguousarray(feature[:, 0]), np.ascontiguousarray(feature[:, 1]), first)

    def BuildTracks(self, reconstruction):
        """Appends the tracks, un-estimated, and their observations to the array-backed Reconstruction."""
        r = reconstruction
        feat_off, pv1, pv2, match_off, f1, f2, first = self.indexed(r.NumViews())
        track_off, obs_view, obs_feature, obs_track, self.stats_ = build_tracks(feat_off, pv1, pv2, match_off, f1, f2, self.options_)
        nt, t0 = len(track_off) - 1, r.NumTracks()
        sides = np.asarray(self.rows_, dtype=np.float64).reshape(-1, 4)[first[feat_off[obs_view] + obs_feature]]
        r.obs_view = np.concatenate([r.obs_view, obs_view]).astype(np.int32)
        r.obs_track = np.concatenate([r.obs_track, obs_track + t0]).astype(np.int32)
        r.obs_uv = np.concatenate([r.obs_uv.reshape(-1, 2), sides[:, :2]])
        r.obs_cov = np.concatenate([r.obs_cov.reshape(-1, 2), sides[:, 2:]])
        for name in ("obs_depth_prior", "obs_depth_prior_variance"):
            if getattr(r, name) is not None:
                setattr(r, name, np.concatenate([getattr(r, name), np.zeros(len(obs_view))]))
        r.points = np.concatenate([r.points, np.zeros((nt, 4))])                      # Track::Track(): point_.setZero()
        r.track_estimated = np.concatenate([r.track_estimated, np.zeros(nt, bool)])
        r.track_reference_view = np.concatenate([r.track_reference_view, obs_view[track_off[:-1]].astype(np.int64)])
        r.inverse_depth = np.concatenate([r.inverse_depth, np.zeros(nt)])
        r.track_reference_bearing = np.concatenate([r.track_reference_bearing, np.zeros((nt, 3))])

    def BuildTracksIncremental(self, reconstruction):
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_UNSUPPORTED,
                                 "BuildTracksIncremental is not built: it needs the component-to-track map across calls")


def AddFeatureCorrespondencesToTrackBuilder(view_id1, features1, view_id2, features2, track_builder):  # sfm_wrapper.h:56-61
    if len(features1) != len(features2):
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "the number of features in each view must be the same")
    for a, b in zip(features1, features2):
        track_builder.AddFeatureCorrespondence(view_id1, (float(a[0]), float(a[1])), view_id2, (float(b[0]), float(b[1])))


def AddFullFeatureCorrespondencesToTrackBuilder(view_id1, features1, view_id2, features2, track_builder):  # sfm_wrapper.h:64-69
    if len(features1) != len(features2):
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "the number of features in each view must be the same")
    for a, b in zip(features1, features2):
        track_builder.AddFeatureCorrespondence(view_id1, a, view_id2, b)
