"""Sequential restatement, one element at a time, of the three reference functions behind csrc/covisibility.hip under the
rules include/theia_hip.h states: ViewGraphFromReconstruction (ascending view index, both views estimated, strict >),
ViewSelectionMVSNet (math.acos / math.exp, a plain ascending sum, no clamp; ties by view index, NaN last, nothing collapses)
and FindCommonTracksInViews.  Plain Python floats and lists; numpy only carries the arrays in and out."""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16


def tracks_by_view(num_views, obs_view, obs_track):
    """every view's tracks, ascending"""
    lists = [[] for _ in range(num_views)]
    for v, t in zip(np.asarray(obs_view).tolist(), np.asarray(obs_track).tolist()):
        lists[v].append(t)
    return [sorted(l) for l in lists]


def intersect(a, b):
    """std::set_intersection of two ascending lists"""
    out, x, y = [], 0, 0
    while x < len(a) and y < len(b):
        if a[x] < b[y]:
            x += 1
        elif b[y] < a[x]:
            y += 1
        else:
            out.append(a[x]); x += 1; y += 1
    return out


def _flag(flags, n):
    return [True] * n if flags is None else [bool(f) for f in np.asarray(flags).tolist()]


def angle_axis_to_rot(aa):
    """ceres::AngleAxisToRotationMatrix, rows of a row-major matrix"""
    x, y, z = aa
    theta2 = x * x + y * y + z * z
    if theta2 > DBL_EPSILON:
        theta = math.sqrt(theta2)
        wx, wy, wz = x / theta, y / theta, z / theta
        c, s = math.cos(theta), math.sin(theta)
        return [[c + wx * wx * (1.0 - c), wx * wy * (1.0 - c) - wz * s, wy * s + wx * wz * (1.0 - c)],
                [wz * s + wx * wy * (1.0 - c), c + wy * wy * (1.0 - c), -wx * s + wy * wz * (1.0 - c)],
                [-wy * s + wx * wz * (1.0 - c), wx * s + wy * wz * (1.0 - c), c + wz * wz * (1.0 - c)]]
    return [[1.0, -z, y], [z, 1.0, -x], [-y, x, 1.0]]


def rot_to_angle_axis(R):
    """ceres::RotationMatrixToAngleAxis through the quaternion (Ceres 2.2)"""
    q = [0.0] * 4
    trace = R[0][0] + R[1][1] + R[2][2]
    if trace >= 0.0:
        t = math.sqrt(trace + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (R[2][1] - R[1][2]) * t; q[2] = (R[0][2] - R[2][0]) * t; q[3] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = math.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
        q[i + 1] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k][j] - R[j][k]) * t
        q[j + 1] = (R[j][i] + R[i][j]) * t
        q[k + 1] = (R[k][i] + R[i][k]) * t
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if s2 > 0.0:
        st, ct = math.sqrt(s2), q[0]
        two_theta = 2.0 * (math.atan2(-st, -ct) if ct < 0.0 else math.atan2(st, ct))
        k = two_theta / st
        return [q[1] * k, q[2] * k, q[3] * k]
    return [q[1] * 2.0, q[2] * 2.0, q[3] * 2.0]


def _div(a, b):
    """a / b as IEEE does it: 0 / 0 and x / 0 do not raise"""
    if b == 0.0:
        return math.nan if (a == 0.0 or math.isnan(a)) else math.copysign(math.inf, a)
    return a / b


def two_view_info(ext_i, ext_j):
    """CreateTwoViewInfo: (rotation_2, position_2) of view j against view i; ext = position | angle-axis"""
    Ri, Rj = angle_axis_to_rot(ext_i[3:6]), angle_axis_to_rot(ext_j[3:6])
    R = [[(Rj[r][0] * Ri[c][0] + Rj[r][1] * Ri[c][1]) + Rj[r][2] * Ri[c][2] for c in range(3)] for r in range(3)]
    d = [ext_j[0] - ext_i[0], ext_j[1] - ext_i[1], ext_j[2] - ext_i[2]]
    n = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    u = [_div(d[0], n), _div(d[1], n), _div(d[2], n)]
    return rot_to_angle_axis(R), [(Ri[r][0] * u[0] + Ri[r][1] * u[1]) + Ri[r][2] * u[2] for r in range(3)]


def view_graph(num_views, num_tracks, obs_view, obs_track, view_estimated, track_estimated, min_shared_tracks, cam_ext=None):
    """-> (pairs [E][2] int32 ascending, num_shared [E] int32, rotation_2 [E][3], position_2 [E][3]); the last two None
    without cam_ext"""
    ve, te = _flag(view_estimated, num_views), _flag(track_estimated, num_tracks)
    est = [[t for t in l if te[t]] for l in tracks_by_view(num_views, obs_view, obs_track)]
    pairs, shared, rot, pos = [], [], [], []
    cam = None if cam_ext is None else np.asarray(cam_ext, dtype=np.float64).reshape(-1, 6).tolist()
    for i in range(num_views):
        if not ve[i]:
            continue
        for j in range(i + 1, num_views):
            if not ve[j]:
                continue
            n = len(intersect(est[i], est[j]))
            if n > min_shared_tracks:
                pairs.append((i, j)); shared.append(n)
                if cam is not None:
                    w, p = two_view_info(cam[i], cam[j])
                    rot.append(w); pos.append(p)
    out = (np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(shared, dtype=np.int32))
    if cam is None:
        return out + (None, None)
    return out + (np.array(rot, dtype=np.float64).reshape(-1, 3), np.array(pos, dtype=np.float64).reshape(-1, 3))


def angle_between_rays(ci, cj, X):
    """ComputeAngleBetweenRays on the homogeneous point X, degrees; no clamp of the cosine: math.acos raises beyond 1,
    which the reference turns into NaN"""
    p = [_div(X[0], X[3]), _div(X[1], X[3]), _div(X[2], X[3])]
    a = [ci[0] - p[0], ci[1] - p[1], ci[2] - p[2]]; b = [cj[0] - p[0], cj[1] - p[1], cj[2] - p[2]]
    na = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); nb = math.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
    c = (_div(a[0], na) * _div(b[0], nb) + _div(a[1], na) * _div(b[1], nb)) + _div(a[2], na) * _div(b[2], nb)
    if math.isnan(c) or abs(c) > 1.0:
        return math.nan
    return 180.0 / math.pi * math.acos(c)


def score_fun(theta, theta0, sigma1, sigma2):
    sigma = sigma1 if theta <= theta0 else sigma2
    d = theta - theta0
    return math.exp(-(d * d) / (2.0 * (sigma * sigma)))


def pair_scores(num_views, obs_view, obs_track, cam_ext, points, pairs, theta0, sigma1, sigma2, track_mask=None):
    """-> (score [E], num_common [E], smallest theta over all terms)"""
    lists = tracks_by_view(num_views, obs_view, obs_track)
    cam = np.asarray(cam_ext, dtype=np.float64).reshape(-1, 6).tolist()
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4).tolist()
    mask = None if track_mask is None else [bool(m) for m in np.asarray(track_mask).tolist()]
    score, common, smallest = [], [], math.inf
    for i, j in np.asarray(pairs).reshape(-1, 2).tolist():
        lo, hi = min(i, j), max(i, j)
        s, n = 0.0, 0
        for t in intersect(lists[lo], lists[hi]):
            if mask is not None and not mask[t]:
                continue
            theta = angle_between_rays(cam[lo][:3], cam[hi][:3], pts[t])
            smallest = min(smallest, theta) if not math.isnan(theta) else smallest
            s += score_fun(theta, theta0, sigma1, sigma2)
            n += 1
        score.append(s); common.append(n)
    return np.array(score, dtype=np.float64), np.array(common, dtype=np.int32), smallest


def order_key(score, view):
    """the selection's order: score descending, NaN after every number, equal scores by ascending view index"""
    return (1, 0.0, view) if math.isnan(score) else (0, -score, view)


def view_selection(num_views, num_tracks, obs_view, obs_track, view_estimated, track_estimated, cam_ext, points,
                   num_neighbors, theta0, sigma1, sigma2, min_shared_tracks=10):
    """-> {view: [(score, neighbour), ...]} for every estimated view, ALL its neighbours in the selection's order; the
    caller cuts at num_neighbors (kept whole so that the scene's score gaps can be checked)"""
    pairs, _, _, _ = view_graph(num_views, num_tracks, obs_view, obs_track, view_estimated, track_estimated, min_shared_tracks)
    score, _, _ = pair_scores(num_views, obs_view, obs_track, cam_ext, points, pairs, theta0, sigma1, sigma2)
    ve = _flag(view_estimated, num_views)
    rows = {v: [] for v in range(num_views) if ve[v]}
    for (i, j), s in zip(pairs.tolist(), score.tolist()):
        rows[i].append((s, j)); rows[j].append((s, i))
    return {v: sorted(r, key=lambda it: order_key(it[0], it[1])) for v, r in rows.items()}


def find_common_tracks(num_views, obs_view, obs_track, queries):
    lists = tracks_by_view(num_views, obs_view, obs_track)
    out = []
    for q in queries:
        q = list(q)
        assert len(q) > 1   # CHECK_GT
        common = lists[q[0]]
        for v in q[1:]:
            if not common:
                break
            common = intersect(common, lists[v])
        out.append(list(common))
    return out
