"""One-element-at-a-time restatements of the reference functions behind pytheiasfm_amd/incremental.py, written from the
reference's text with plain loops and Python ints; nothing of pytheiasfm_amd decides a result here.

  VisibilityPyramid                         sfm/visibility_pyramid.cc:47-103
  find_views_to_localize                    sfm/incremental_reconstruction_estimator.cc:422-463
  set_underconstrained_{views,tracks,as}    sfm/reconstruction_estimator_utils.cc:291-350, incremental_reconstruction_estimator.cc:612-620
  order_view_pairs                          sfm/incremental_reconstruction_estimator.cc:384-420

A reconstruction is passed as plain sequences: obs_view / obs_track / obs_uv rows, flag lists, (width, height) rows."""


def clamp(v, lo, hi):
    return max(lo, min(hi, v))


class VisibilityPyramid:
    def __init__(self, width, height, num_pyramid_levels):
        assert width > 0 and height > 0 and num_pyramid_levels > 0          # CHECK_GT (:54-56)
        self.width, self.height = int(width), int(height)
        self.max_cells = 1 << num_pyramid_levels
        # level i: a set of occupied (x, y) of a grid with 1 << (1 + i) cells per side (:60-64); count() only asks "non-zero"
        self.pyramid = [set() for _ in range(num_pyramid_levels)]

    def add_point(self, x, y):
        # static_cast<int>(max_cells * x / width) (:71-78).  Python's int() truncates toward zero like the cast and has no
        # range: where the C++ cast is undefined (a quotient outside int) this is the clamp of the exact truncation, which
        # is what the library defines
        gx = clamp(int(self.max_cells * float(x) / self.width), 0, self.max_cells - 1)
        gy = clamp(int(self.max_cells * float(y) / self.height), 0, self.max_cells - 1)
        for i in range(len(self.pyramid) - 1, -1, -1):                      # :82-90
            self.pyramid[i].add((gx, gy))
            gx >>= 1
            gy >>= 1

    def compute_score(self):
        score = 0
        for i, level in enumerate(self.pyramid):                            # :97-103: count() * size()
            side = 1 << (1 + i)
            score += len(level) * side * side
        return score


def view_rows(obs_view, view_id):
    """A view's observations in array order."""
    return [k for k in range(len(obs_view)) if obs_view[k] == view_id]


def view_score(obs_view, obs_track, obs_uv, track_estimated, size, view_id, levels):
    """(number of estimated tracks, pyramid score) of one view (:437-447)."""
    pyramid = VisibilityPyramid(size[0], size[1], levels)
    n = 0
    for k in view_rows(obs_view, view_id):
        if track_estimated[obs_track[k]]:
            n += 1
            pyramid.add_point(obs_uv[k][0], obs_uv[k][1])
    return n, pyramid.compute_score()


def find_views_to_localize(obs_view, obs_track, obs_uv, track_estimated, image_size, unlocalized_views, min_points=30, levels=6):
    scores = []
    for v in unlocalized_views:
        n, s = view_score(obs_view, obs_track, obs_uv, track_estimated, image_size[v], v, levels)
        if n >= min_points:                                                  # :451
            scores.append((s, int(v)))
    scores.sort(reverse=True)                                                # std::greater<std::pair<int, ViewId>>
    return [v for _, v in scores]


def set_underconstrained_tracks(obs_view, obs_track, view_estimated, track_estimated):
    """:291-319, in place; returns the count."""
    removed = 0
    for t in range(len(track_estimated)):
        if not track_estimated[t]:
            continue
        n = 0
        for k in range(len(obs_track)):
            if obs_track[k] == t and view_estimated[obs_view[k]]:
                n += 1
            if n >= 2:
                break
        if n < 2:
            track_estimated[t] = False
            removed += 1
    return removed


def set_underconstrained_views(obs_view, obs_track, view_estimated, track_estimated):
    """:321-350, in place; returns the count."""
    removed = 0
    for v in range(len(view_estimated)):
        if not view_estimated[v]:
            continue
        n = 0
        for k in range(len(obs_view)):
            if obs_view[k] == v and track_estimated[obs_track[k]]:
                n += 1
            if n >= 3:
                break
        if n < 3:
            view_estimated[v] = False
            removed += 1
    return removed


def _by_index(index, n):
    rows = [[] for _ in range(n)]
    for k, i in enumerate(index):
        rows[i].append(k)
    return rows


def set_underconstrained_as_unestimated(obs_view, obs_track, view_estimated, track_estimated):
    """incremental_reconstruction_estimator.cc:612-620, in place -> (views removed, tracks removed, rounds).  The passes are
    the two functions above with the observations bucketed once (the scans above are quadratic; the counts are the same)."""
    by_view = _by_index(obs_view, len(view_estimated))
    by_track = _by_index(obs_track, len(track_estimated))
    num_views, num_tracks = -1, -1
    total_views = total_tracks = rounds = 0
    while num_views != 0 and num_tracks != 0:
        num_views = 0
        for v in range(len(view_estimated)):
            if view_estimated[v] and sum(1 for k in by_view[v] if track_estimated[obs_track[k]]) < 3:
                view_estimated[v] = False
                num_views += 1
        num_tracks = 0
        for t in range(len(track_estimated)):
            if track_estimated[t] and sum(1 for k in by_track[t] if view_estimated[obs_view[k]]) < 2:
                track_estimated[t] = False
                num_tracks += 1
        total_views += num_views
        total_tracks += num_tracks
        rounds += 1
    return total_views, total_tracks, rounds


def order_view_pairs(view_pairs, min_num_verified_matches):
    """:384-420.  view_pairs: [((id1, id2), num_verified_matches, num_homography_inliers)]."""
    crit = []
    for pair, verified, homography in view_pairs:
        if verified > min_num_verified_matches:
            crit.append((homography, -verified, pair))
    crit.sort()
    return [c[2] for c in crit]
