"""theia_hip_estimate_tracks' triangulation stage (k_track_triangulate, triangulate_nview, track_projection_matrix,
smallest_eigenvector4) and theia_hip_track_statistics (k_track_stats) against the plain references of tests/triangulation_ref.py,
on the track cuts of tests/triangulation_scenes.py: all eight camera models, skew and aspect ratio in use, the zero and the 1e-9
rotation camera, scaled and negated homogeneous points, tracks of 0, 1, 2 .. 10 and 65 observations, and for the pinhole model the
tracks built by hand (a singular midpoint system, a track that passes the angle test on its last pair only, a pair on either side
of the angle threshold).

Tolerances are per track and come from the reference alone: c N eps ||M||_2 / gap for the two eigenvector methods and
c N eps cond(A) for the midpoint, with c = 10 max(c_np, 1) = 10, c_np being what float64 numpy shows against mpmath on the same
tracks (eigh 0.25, svd 1.3e-4, solve 0.77: test_triangulation_ref.py).  Largest device ratio seen on an MI355X: L2 0.16, SVD 3.2e-4,
midpoint 0.74.

The SVD cases found the kernel returning the L2 vector on well-conditioned tracks (tracks 18 and 26 of the fisheye cut, 35 of the
extended-unified cut: error 0.9, bound 5e-10): its mu iteration never met |dmu| <= 1e-13 mu at the rounding floor of mu.  Fixed in
triangulate_nview (it also stops once the steps are below 1e-10 mu and no longer shrink)."""
import functools

import numpy as np
import pytest

from pytheiasfm_amd import ba
from tests import ba_edge_scenes as es
from tests import oracle_lib as ol
from tests import triangulation_ref as tr
from tests import triangulation_scenes as ts

pytestmark = pytest.mark.gpu

METHODS = {0: "midpoint", 1: "svd", 2: "l2"}
COMPARABLE = 0.1       # (test_triangulation_ref.py: above this a unit vector has no direction to compare -- the antiparallel track)
COUNTERS = ("bad_angles", "failed_triangulations", "bad_reprojections", "ba_failures")


def options(side="gpu", pd=3, iters=15):
    o = ba.default_options() if side == "gpu" else ol.default_options()
    o.max_num_iterations = iters
    o.use_inner_iterations = 0
    o.use_homogeneous_point_parametrization = 1 if pd == 3 else 0
    return o


@functools.lru_cache(maxsize=None)
def device_rays(model, name="cut"):
    v = ts.variant(model, name)
    if name in ("interleaved", "double"):
        d = device_rays(model, "cut")[v.parent].copy()        # row for row the rays of the cut: the comparison is of bits
        return d
    if name == "far":
        return device_rays(model, "cut")
    return ts.rays(v)


def run(model, name, method, bundle=False, pd=3, problem=None, rays=None):
    p = (ts.variant(model, name).p if problem is None else problem).copy()
    est, cnt = ba.estimate_tracks(p, device_rays(model, name) if rays is None else rays, options("gpu", pd), ts.MIN_ANGLE_DEG, 5.0, bundle,
                                  triangulation_method=method)
    return p.points, est, cnt


@functools.lru_cache(maxsize=None)
def triangulated(model, name, method):
    return run(model, name, method)


@functools.lru_cache(maxsize=None)
def angle_ok(model, name="cut"):
    v = ts.variant(model, name)
    d = device_rays(model, name)
    return np.array([tr.sufficient_angle(d[v.p.obs_pt == t], ts.MIN_ANGLE_DEG) for t in range(v.p.points.shape[0])])


@functools.lru_cache(maxsize=None)
def midpoint_refs(model, name):
    v = ts.variant(model, name)
    return tr.midpoint_references(v.p, device_rays(model, name))


# ---------------------------------------------------------------- projection matrix and the two linear methods
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("model", ts.MODELS)
def test_linear_methods_against_mpmath(model, method):
    """Without the track BA the point is TriangulateNViewSVD / TriangulateNView of the pixels and the projection matrices: the
    4-vector against mpmath up to sign, within 10 N eps ||M|| / gap per track.  For SVD the vector must be the SVD reference's:
    on the tracks where the L2 reference is further away than the bound that also shows that nothing fell back."""
    kind = METHODS[method]
    pts, est, cnt = triangulated(model, "cut", method)
    ok = angle_ok(model)
    worst, compared, told_apart, fails = 0.0, 0, 0, []
    for t, ref in tr.cut_references(model).items():
        tol = tr.eigen_tolerance(ref[kind], tr.device_c(kind))
        if not ok[t] or not tol < COMPARABLE:
            continue
        err = tr.sign_error(pts[t], ref[kind]["x"])
        compared += 1
        worst = max(worst, err / tr.eigen_tolerance(ref[kind], 1.0))
        if not err <= tol:
            fails.append("track %d (%d views): error %.3e, bound %.3e" % (t, ref[kind]["N"], err, tol))
        if method == 1:
            other = ref["l2"]["x"] * np.linalg.norm(ref["svd"]["x"])
            told_apart += tr.sign_error(other, ref["svd"]["x"]) > 2.0 * tol
    print("model %d %s: %d tracks compared, largest error / (N eps ||M|| / gap) = %.3g; L2 told apart on %d" % (model, kind, compared, worst, told_apart))
    assert not fails, "\n".join(fails)
    assert compared >= 47 + (3 if model == 0 else 0)
    assert method != 1 or told_apart >= compared // 2
    assert cnt["failed_triangulations"] == 0
    assert np.isfinite(pts).all()
    assert np.array_equal(pts[~ok], np.tile([0.0, 0.0, 0.0, 1.0], (int((~ok).sum()), 1)))


# ---------------------------------------------------------------- midpoint
@pytest.mark.parametrize("name", ["cut", "far"])
@pytest.mark.parametrize("model", ts.MODELS)
def test_midpoint_against_mpmath(model, name):
    """The midpoint against the 3 x 3 solve in mpmath, within 10 N eps cond(A) relative to max(1, |X|), also with cameras and points
    moved by (1e4, -2e4, 5e3) (b = sum (I - d d^T) o then cancels five digits)."""
    v = ts.variant(model, name)
    pts, est, cnt = triangulated(model, name, 0)
    ok = angle_ok(model, name)
    rays = device_rays(model, name)
    worst, worst_np, compared = 0.0, 0.0, 0
    for t, ref in midpoint_refs(model, name).items():
        if not ok[t]:
            continue
        if ref["X"] is None:
            assert model == 0 and t == v.hand["antiparallel"]
            continue
        sel = np.flatnonzero(v.p.obs_pt == t)
        scale = max(1.0, np.linalg.norm(ref["X"]))
        assert pts[t, 3] == 1.0
        worst = max(worst, np.linalg.norm(pts[t, :3] - ref["X"]) / scale / tr.midpoint_tolerance(ref, 1.0))
        worst_np = max(worst_np, np.linalg.norm(tr.numpy_midpoint(v.p.cam_ext[v.p.obs_cam[sel], :3], rays[sel]) - ref["X"]) / scale / tr.midpoint_tolerance(ref, 1.0))
        compared += 1
    print("model %d %s: %d tracks, error / (N eps cond): device %.3g, numpy %.3g" % (model, name, compared, worst, worst_np))
    assert compared >= 48 and worst_np <= tr.C_NP["midpoint"]
    assert worst <= tr.device_c("midpoint")
    if name == "far":
        assert np.abs(pts[ok & (pts[:, 3] == 1.0) & est, :3] - ts.FAR).max() < 10.0
    else:      # the triangulated points stand at the truth (0.5 px noise; the hand-built tracks are exact)
        done = ok & (est if model != 7 else np.zeros_like(est))      # (an orthographic camera leaves the depth to the other views)
        assert not done.any() or np.median(np.abs(pts[done, :3] - v.truth[done, :3] / v.truth[done, 3:]).max(1)) < 0.05


# ---------------------------------------------------------------- counters and decisions
@pytest.mark.parametrize("bundle", [False, True])
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("model", ts.MODELS)
def test_counters_and_decisions(model, method, bundle):
    """Every track ends in exactly one place: a counter, `estimated`, or (constant) nowhere.  The tracks that fail the angle test on
    the supplied rays are the bad angles and keep their bits; on the pinhole cut the tracks built by hand fall where they were
    built to fall."""
    cut = ts.track_cut(model)
    p = cut.p.copy()
    n = p.points.shape[0]
    const = [7, cut.names["long"]]
    p.point_const = np.zeros(n, np.uint8); p.point_const[const] = 1
    p.points[const[0]] = [1.5, -2.25, 3.125, 0.5]
    p.points[const[1]] = [-0.0, 5e-324, 1e300, -1.0]
    before = p.points.copy()
    pts, est, cnt = run(model, "cut", method, bundle, problem=p)
    ok = angle_ok(model).copy()
    ok[const] = True
    h = cut.hand
    failed = [h["antiparallel"]] if (model == 0 and method == 0) else []
    assert cnt["bad_angles"] == int((~ok).sum()) == (3 if model == 0 else 0)
    assert cnt["failed_triangulations"] == len(failed)
    assert sum(cnt[k] for k in COUNTERS) + int(est.sum()) + len(const) == n
    assert not est[~ok].any() and not est[failed].any() and not est[const].any()
    untouched = sorted(set(np.flatnonzero(~ok).tolist()) | set(failed) | set(const))
    assert before[untouched].tobytes() == pts[untouched].tobytes()
    assert np.isfinite(pts[est]).all()
    moved = np.ones(n, bool); moved[untouched] = False
    if model == 0:      # (with the linear methods the antiparallel track is "triangulated": some vector of a two-dimensional null space)
        moved[h["antiparallel"]] = False
    assert (np.abs(pts[moved] - before[moved]).max(1) > 0.0).all()
    if model == 0:
        assert not est[h["below"]] and not est[h["one_view"]] and not est[h["no_view"]] and not ok[h["below"]]
        for name in ("last_pair", "last_pair_only", "above"):
            assert est[h[name]] and np.abs(pts[h[name], :3] / pts[h[name], 3] - cut.truth[h[name], :3]).max() < 1e-6, name
    if (bundle or method == 0) and not few_tracks_pass(model, method):    # (the linear methods ignore the distortion: without the BA they may fail the 5 px test)
        assert est.sum() >= n - len(const) - 3 - 3


# ---------------------------------------------------------------- order and batch shape
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("model", ts.MODELS)
def test_interleaved_observations_give_the_same_bits(model, method):
    """group_by_point and the ray permutation: the observation arrays permuted so that tracks interleave (rays with them) give
    bit-identical points, `estimated` and counters, track BA included."""
    a = run(model, "cut", method, True)
    b = run(model, "interleaved", method, True)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].sum() >= (1 if few_tracks_pass(model, method) else 40)


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("model", ts.MODELS)
def test_batches_of_1_64_65_tracks_give_the_bits_of_the_full_batch(model, method):
    """The cut followed by its far copy (2 x the tracks, a partly filled second workgroup; a single cut has fewer than 65 tracks): its
    first 1, 64 and 65 tracks as batches of their own give, per track, the bits of the full batch."""
    v = ts.variant(model, "double")
    full = run(model, "double", method, True)
    assert v.p.points.shape[0] > 65
    for n in (1, 64, 65):
        q, rows = ts.first_tracks(v, n)
        pts, est, cnt = run(model, "double", method, True, problem=q, rays=np.ascontiguousarray(device_rays(model, "double")[rows]))
        assert pts.tobytes() == full[0][:n].tobytes() and np.array_equal(est, full[1][:n]), n
        assert sum(cnt[k] for k in COUNTERS) + int(est.sum()) == n


# ---------------------------------------------------------------- with the track BA
def few_tracks_pass(model, method):
    """Where EstimateTrack itself lets few tracks through: an orthographic camera leaves the depth to the other views (the
    triangulated point often lies behind one of them), and TriangulateNView(SVD) ignores the strong distortion of the double-sphere
    groups (the track LM then fails from that start on several tracks)."""
    return model == 7 or (model == 5 and method != 0)


# The number of estimated tracks compared in the cases of few_tracks_pass, as an MI355X shows them: (model, method, pd) -> count.
SEEN = {(5, 1, 3): 16, (5, 1, 4): 16, (5, 2, 3): 16, (5, 2, 4): 16,
        (7, 0, 3): 13, (7, 0, 4): 16, (7, 1, 3): 1, (7, 1, 4): 16, (7, 2, 3): 16, (7, 2, 4): 16}


def lm_tracks(cut, method, pd):
    """The tracks compared, in this order, until 16 estimated ones are seen: the planted ones, one on-axis point, one of the tracks of
    cameras 0 and 1, the 65-observation track, one of every length 3 .. 10; where few tracks pass (few_tracks_pass) the rest of
    the cut after them.  For the orthographic model two kinds of track have no answer to compare with and are left out:

      * the tracks that only cameras 0 and 1 see: both are unrotated, an orthographic projection drops z, so nothing fixes the
        point's z (the oracle ends such a track at |z| of 1e7);
      * with the ambient parametrisation the tracks that only ring cameras see.  Cameras 2 .. 11 look exactly at the origin, so
        R (X - w C) moves along each such axis when w moves: the w column of the Jacobian is the round-off of R C, the cost is
        flat along (0, 0, 0, 1), and the ORACLE's own result moves by 5e-5 .. 5e-2 on 8 of 13 such tracks when the CAMERAS move by
        1e-15 (a move of the start point alone changes it by 2e-12 at most; measured with the oracle alone).  No rule of the
        geometry tells the five stable ones from the others, so all are left out.  Cameras 0 and 1 stand beside their axis and
        fix w."""
    names = cut.names
    p = cut.p
    nedge = p.points.shape[0] - len(cut.hand)
    counts = np.bincount(p.obs_pt, minlength=p.points.shape[0])
    chosen = [names["origin"], names["w_quarter"]] + ([names["w_negative"]] if names["w_negative"] is not None else [])
    chosen += [names["axis"][0], names["pair01"][0], names["long"]]
    for length in range(3, 11):
        chosen.append(next(t for t in range(nedge) if counts[t] == length and t not in chosen))
    assert len(chosen) <= 16
    if few_tracks_pass(cut.model, method):
        chosen += [t for t in range(nedge) if t not in chosen]
    if cut.model == 7:
        cams = lambda t: set(p.obs_cam[p.obs_pt == t].tolist())
        chosen = [t for t in chosen if not cams(t) <= {0, 1} and (pd == 3 or cams(t) & {0, 1})]
    return chosen


@pytest.mark.parametrize("pd", [3, 4])
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("model", ts.MODELS)
def test_track_ba_follows_the_oracle_from_the_triangulated_point(model, method, pd):
    """With the track BA every estimated track ends within 1e-8 max(1, |X|) of the oracle's LM on the one-track problem (cameras
    constant) started from the device's own triangulated point -- the bound of
    test_ba_gpu.test_estimate_tracks_follows_track_estimator_rules -- for the three methods and both point parametrisations.  At
    least 12 tracks are compared per case; where few tracks pass, the count of SEEN."""
    cut = ts.track_cut(model)
    start, _, _ = triangulated(model, "cut", method)
    pts, est, cnt = run(model, "cut", method, True, pd)
    oo = options("oracle", pd)
    worst, fails, seen = 0.0, [], 0
    for t in lm_tracks(cut, method, pd):
        if not est[t]:
            continue
        if seen == 16:
            break
        q = cut.p.copy(); q.points[t] = start[t]
        fp = es.track_slice(q, t)
        so, _ = ol.solve(fp, oo)
        dev = float(np.abs(pts[t] - fp.points[0]).max()) / max(1.0, float(np.abs(fp.points[0]).max()))
        worst = max(worst, dev); seen += 1
        if not (so.success and dev <= 1e-8):
            fails.append("track %d: %.3e (|X| %.3g, oracle success %d, %d iterations)" % (t, dev, np.abs(fp.points[0]).max(), so.success, so.num_iterations))
    print("model %d %s pd %d: %d tracks, worst %.3e, estimated %d, counters %s" % (model, METHODS[method], pd, seen, worst, est.sum(), cnt))
    assert not fails, "\n".join(fails)
    assert seen >= (SEEN[(model, method, pd)] if few_tracks_pass(model, method) else 12)


# ---------------------------------------------------------------- track_statistics as values
@pytest.mark.parametrize("model", ts.MODELS)
def test_track_statistics_values(model):
    """The three outputs of theia_hip_track_statistics as values, at the true points (w = 0.25 and w = -1 among them; cameras 0 and 1
    take the first-order rotation): the mean squared error against the oracle's residuals (1e-11 relative to the largest, the bound
    test_ba_instances_gpu.py has for residuals), the views behind the camera exactly, the minimum ray cosine within 16 eps (2.0
    below two views).  No observation is within 1e-12 |X - w C| of zero depth (asserted; the smallest is 1e-3 and more).  A second
    state puts the points of the tracks of cameras 0 and 1 behind those two cameras: counts and cosines only."""
    cut = ts.track_cut(model)
    q = ts.with_truth(cut)
    counts = np.bincount(q.obs_pt, minlength=q.points.shape[0])
    ok, mse, nb, mincos, margin = tr.track_stats(q)
    assert ok == 1 and margin.min() > 1e-12
    err, behind, mc = ba.track_statistics(q)
    seen = counts > 0
    dev = float(np.abs(err[seen] - mse[seen]).max() / np.abs(mse[seen]).max())
    print("model %d: mse %.3e relative (largest %.3g px^2), behind %d, cosine %.3e" % (model, dev, mse[seen].max(), nb.sum(), np.abs(mc - mincos).max()))
    assert dev <= 1e-11
    assert np.array_equal(behind, nb) and nb.sum() == (1 if model == 0 else 0)
    assert np.abs(mc - mincos).max() <= 16.0 * tr.EPS and np.array_equal(mc == 2.0, counts < 2)
    if model == 0:
        assert behind[cut.hand["antiparallel"]] == 1 and behind[cut.hand["no_view"]] == 0 and mc[cut.hand["one_view"]] == 2.0
    # behind the unrotated cameras
    q2 = q.copy()
    pair = cut.names["pair01"][:10]
    q2.points[pair, 2] = -9.0 - q2.points[pair, 2]
    ok2, _, nb2, mincos2, margin2 = tr.track_stats(q2)
    assert margin2.min() > 1e-12 and (nb2[pair] == 2).all()
    _, behind2, mc2 = ba.track_statistics(q2)
    assert np.array_equal(behind2, nb2) and np.abs(mc2 - mincos2).max() <= 16.0 * tr.EPS
