"""The references and inputs of tests/test_triangulation_gpu.py, checked on the CPU: the mpmath references against numpy and against
the oracle's own midpoint, the projection matrix against the oracle's projection, what each cut claims to contain, and the
condition that the device's mu iteration (restated in numpy) settles on every track of every cut."""
import functools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from tests import ba_edge_scenes as es
from tests import oracle_lib as ol
from tests import triangulation_ref as tr
from tests import triangulation_scenes as ts

# identity value of every distortion slot: (first slot, values)
IDENTITY_DISTORTION = {0: (5, [0.0, 0.0]), 1: (5, [0.0] * 5), 2: (5, [0.0] * 4), 3: (4, [0.0]), 4: (4, [0.0]), 5: (5, [0.0, 0.0]),
                       6: (5, [0.0, 1.0]), 7: (5, [0.0, 0.0])}
COMPARABLE = 0.1     # a unit vector whose tolerance is above this has no direction to compare (the antiparallel track: gap 0)


@functools.lru_cache(maxsize=None)
def numpy_ratios(model):
    """The largest error / (N eps ||M|| / gap) of numpy's eigh and svd, and error / (N eps cond) of numpy's solve and of the
    oracle's midpoint, against mpmath on the tracks of one cut."""
    cut = ts.track_cut(model)
    rays = ts.numpy_rays(cut)
    rules = ol.sfm_rules()
    worst = {"l2": 0.0, "svd": 0.0, "midpoint": 0.0, "midpoint_oracle": 0.0}
    for t, ref in tr.cut_references(model).items():
        Ps, uv, C, sel = tr.track_inputs(cut.p, t)
        for kind, fn in (("l2", tr.numpy_l2), ("svd", tr.numpy_svd)):
            if tr.eigen_tolerance(ref[kind], tr.device_c(kind)) < COMPARABLE:
                worst[kind] = max(worst[kind], tr.sign_error(fn(Ps, uv), ref[kind]["x"]) / tr.eigen_tolerance(ref[kind], 1.0))
        m = tr.midpoint(C, rays[sel])
        if m["X"] is None:
            assert rules._triangulate_midpoint(C, rays[sel]) is None
            continue
        scale = max(1.0, np.linalg.norm(m["X"]))
        worst["midpoint"] = max(worst["midpoint"], np.linalg.norm(tr.numpy_midpoint(C, rays[sel]) - m["X"]) / scale / tr.midpoint_tolerance(m, 1.0))
        Xo = rules._triangulate_midpoint(C, rays[sel])
        worst["midpoint_oracle"] = max(worst["midpoint_oracle"], np.linalg.norm(Xo[:3] / Xo[3] - m["X"]) / scale / tr.midpoint_tolerance(m, 1.0))
    return worst


@pytest.mark.parametrize("model", ts.MODELS)
def test_references_agree_and_numpy_constants(model):
    """nview_l2 against numpy.linalg.eigh, nview_svd against numpy.linalg.svd, midpoint against numpy's solve and against
    oracle/sfm_rules._triangulate_midpoint, up to sign, each inside its own per-track bound with c = C_NP.  Measured over the
    eight cuts (largest ratio): eigh 0.25, svd 1.3e-4, solve 0.77, the oracle's LLT 0.97 -- all below 1, so C_NP = 1 and
    the device is allowed c = 10."""
    w = numpy_ratios(model)
    print("model %d: numpy / mpmath ratios %s" % (model, {k: "%.3g" % v for k, v in w.items()}))
    assert 0.0 < w["l2"] <= tr.C_NP["l2"] and 0.0 < w["svd"] <= tr.C_NP["svd"]
    assert 0.0 < w["midpoint"] <= tr.C_NP["midpoint"] and 0.0 < w["midpoint_oracle"] <= tr.C_NP["midpoint"]


def test_long_track_path_of_the_reference_equals_the_full_decomposition():
    """The inverse iteration that the 65-observation track takes gives what mpmath's full eigen-decomposition gives (on a
    10-observation track forced down that path)."""
    import mpmath
    cut = ts.track_cut(1)
    t = int(np.flatnonzero(np.bincount(cut.p.obs_pt) == 10)[0])
    Ps, uv, _, _ = tr.track_inputs(cut.p, t)
    with mpmath.mp.workdps(tr.DPS):
        A = tr._mpm(tr.svd_matrix(Ps, uv)); M = A.T * A
        E, Q = mpmath.mp.eigsy(M)
        order = sorted(range(M.rows), key=lambda i: E[i])
        big = mpmath.mp.zeros(17, 17)          # the same matrix padded by three large decoupled eigenvalues: 17 rows take the iteration
        for i in range(14):
            for j in range(14):
                big[i, j] = M[i, j]
        for i in range(14, 17):
            big[i, i] = mpmath.mpf(10) ** 12
        l0, l1, v = tr._two_smallest(big)
        assert abs(l0 - E[order[0]]) <= mpmath.mpf(10) ** -40 * abs(E[order[0]]) and abs(l1 - E[order[1]]) <= mpmath.mpf(10) ** -10 * abs(E[order[1]])
        assert tr.sign_error(tr._vec(v)[:14], tr._vec(Q[:, order[0]])) < 1e-30


@pytest.mark.parametrize("model", ts.MODELS)
def test_projection_matrix_against_the_oracles_projection(model):
    """With every distortion slot at its identity value the oracle's projection of a point is the dehomogenised P X (1e-9 px).
    Intrinsics: the scene's three groups (skew -0.1 .. 0.2, aspect 0.98 .. 1.02 where the model has the slots).  The fisheye
    model is equidistant (r = f theta) even without distortion, so its points stay within 1.2e-4 rad of the axis, where
    f (tan(theta) - theta) is below 4e-10 px (and x^2 + y^2 above the 1e-8 under which the model copies x and y); the orthographic model does not divide by z, so its points stand at z = 1."""
    rng = np.random.default_rng(0x9A7 + model)
    cams = es._ring()
    intr = np.zeros((3, capi.THEIA_MAX_INTRINSICS))
    for g in range(3):
        k = list(es.INTRINSICS[model][g])
        first, ident = IDENTITY_DISTORTION[model]
        k[first:first + len(ident)] = ident
        intr[g, :len(k)] = k
    if model not in tr.NO_SKEW_MODELS:
        assert (intr[:, 2] != 0.0).any()
    assert (intr[:, 1] != 1.0).any()
    pts, oc = [], []
    for c in range(es.NV):
        R = tr.rotation_matrix(cams[c, 3:])
        for _ in range(6):
            if model == 2:
                q = np.array([rng.choice([-1.0, 1.0]) * (1.5e-4 + 2.5e-4 * rng.random()), rng.choice([-1.0, 1.0]) * (1.5e-4 + 2.5e-4 * rng.random()), 5.0])
            elif model == 7:
                q = np.array([4.0 * rng.random() - 2.0, 4.0 * rng.random() - 2.0, 1.0])
            else:
                q = np.array([0.6 * rng.random() - 0.3, 0.6 * rng.random() - 0.3, 1.0]) * (3.0 + 4.0 * rng.random())
            pts.append(np.append(cams[c, :3] + R.T @ q, 1.0)); oc.append(c)
    n = len(pts)
    p = capi.FlatProblem(cams, intr, [model] * 3, np.arange(es.NV, dtype=np.int32) % 3, np.array(pts), np.zeros((n, 2)), np.asarray(oc, np.int32),
                         np.arange(n, dtype=np.int32))
    ok, uv = es.project_with_oracle(p, p.cam_ext, p.points)
    assert ok == 1
    worst = 0.0
    for i in range(n):
        c = oc[i]
        x = tr.projection_matrix(model, intr[c % 3], cams[c]) @ p.points[i]
        worst = max(worst, np.abs(x[:2] / x[2] - uv[i]).max())
    print("model %d: |P X - oracle| max %.2e px over %d points" % (model, worst, n))
    assert worst <= 1e-9
    assert np.abs(uv - intr[p.cam_group[p.obs_cam]][:, [2, 3] if model in tr.NO_SKEW_MODELS else [3, 4]]).max() > (1e-3 if model == 2 else 10.0)


@pytest.mark.parametrize("model", ts.MODELS)
def test_cut_contains_what_it_claims(model):
    cut = ts.track_cut(model)
    p = cut.p
    counts = np.bincount(p.obs_pt, minlength=p.points.shape[0])
    nedge = p.points.shape[0] - len(cut.hand)
    assert nedge <= ts.MAX_EDGE_TRACKS
    assert set(range(2, 11)) | {65} <= set(counts[:nedge].tolist()) and counts[cut.names["long"]] == 65
    assert np.array_equal(p.points, np.tile([0.0, 0.0, 0.0, 1.0], (p.points.shape[0], 1)))
    th2 = (p.cam_ext[:, 3:] ** 2).sum(1)
    assert th2[0] == 0.0 and 0.0 < th2[1] <= tr.EPS and (th2[2:12] > tr.EPS).all()
    for t in cut.names["pair01"][:10]:
        assert sorted(p.obs_cam[p.obs_pt == t].tolist()) == [0, 1]
    used = p.intrinsics[p.cam_group[np.unique(p.obs_cam)]]
    assert (used[:, 1] != 1.0).any()
    assert model in tr.NO_SKEW_MODELS or (used[:, 2] != 0.0).any()
    assert np.all(cut.truth[cut.names["origin"], :3] == 0.0) and cut.truth[cut.names["w_quarter"], 3] == 0.25
    assert (cut.names["w_negative"] is not None) == (model in es.NEGATIVE_W_MODELS)
    if model in es.NEGATIVE_W_MODELS:
        assert cut.truth[cut.names["w_negative"], 3] == -1.0
    # one on-axis point per group, on the axis of cameras 2, 3, 4
    q = es.camera_frame(p.cam_ext, cut.truth, p.obs_cam, p.obs_pt)
    for t, c in zip(cut.names["axis"], (2, 3, 4)):
        row = np.flatnonzero((p.obs_pt == t) & (p.obs_cam == c))
        assert len(row) == 1 and q[row[0], 0] ** 2 + q[row[0], 1] ** 2 < 1e-16
    # every observation that is kept sees its point in front of the camera (the antiparallel track's second camera apart)
    depth = q[:, 2] / cut.truth[p.obs_pt, 3]
    behind = np.flatnonzero(depth <= 0.0)
    assert [int(p.obs_pt[i]) for i in behind] == ([cut.hand["antiparallel"]] if model == 0 else [])
    # the statistics tests need no exclusion of a depth at rounding level
    ok, mse, nb, mincos, margin = tr.track_stats(ts.with_truth(cut))
    assert ok == 1 and margin.min() > 1e-3 and np.isfinite(mse[counts > 0]).all()
    assert np.array_equal(mincos == 2.0, counts < 2)
    # the interleaved variant: the same multiset of observations, tracks interleaved, each track in its own order
    iv = ts.variant(model, "interleaved")
    assert (np.diff(iv.p.obs_pt) < 0).sum() >= 9 and (np.diff(iv.p.obs_pt[:40]) > 0).all()      # one descent per round of the round-robin
    for t in range(p.points.shape[0]):
        a, b = np.flatnonzero(p.obs_pt == t), np.flatnonzero(iv.p.obs_pt == t)
        assert np.array_equal(p.obs_uv[a], iv.p.obs_uv[b]) and np.array_equal(p.obs_cam[a], iv.p.obs_cam[b]) and np.array_equal(iv.parent[b], a)


def test_hand_built_tracks_stand_where_they_should():
    cut = ts.track_cut(0)
    p, h = cut.p, cut.hand
    rays = ts.numpy_rays(cut)
    counts = np.bincount(p.obs_pt, minlength=p.points.shape[0])
    assert [int(counts[h[k]]) for k in ("antiparallel", "last_pair", "last_pair_only", "above", "below", "one_view", "no_view")] == [2, 6, 6, 2, 2, 1, 0]
    cos3 = np.cos(np.deg2rad(ts.MIN_ANGLE_DEG))
    d = rays[p.obs_pt == h["antiparallel"]]
    assert np.array_equal(d, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]) and tr.midpoint(p.cam_ext[p.obs_cam[p.obs_pt == h["antiparallel"]], :3], d)["X"] is None
    A = sum(np.eye(3) - np.outer(v, v) for v in d)
    assert np.array_equal(A, np.diag([2.0, 2.0, 0.0]))
    d = rays[p.obs_pt == h["last_pair"]]
    G = d @ d.T
    assert (G[:5, :5] >= cos3).all() and (G[:5, 5] < cos3).all() and abs(np.rad2deg(np.arccos(G[0, 5])) - 10.0) < 1e-6
    d = rays[p.obs_pt == h["last_pair_only"]]
    passing = np.argwhere(np.triu(d @ d.T < cos3, 1))
    assert passing.tolist() == [[4, 5]]
    for name, sign in (("above", -1.0), ("below", 1.0)):      # above the angle: below the cosine
        d = rays[p.obs_pt == h[name]]
        dot = (d[0, 0] * d[1, 0] + d[0, 1] * d[1, 1]) + d[0, 2] * d[1, 2]
        assert sign * (dot - cos3) > 64.0 * tr.EPS and abs(dot - cos3) < 1e-11
        assert tr.sufficient_angle(d, ts.MIN_ANGLE_DEG) == (name == "above")
    assert not tr.sufficient_angle(rays[p.obs_pt == h["one_view"]], 3.0) and not tr.sufficient_angle(rays[p.obs_pt == h["no_view"]], 3.0)
    # every other track of every cut passes the angle test on the true rays
    for model in ts.MODELS:
        c = ts.track_cut(model)
        r = ts.numpy_rays(c)
        for t in range(c.p.points.shape[0] - len(c.hand)):
            assert tr.sufficient_angle(r[c.p.obs_pt == t], ts.MIN_ANGLE_DEG), (model, t)
    # the far variant moves cameras and truth together
    far = ts.variant(0, "far")
    assert np.allclose(far.p.cam_ext[:, :3] - p.cam_ext[:, :3], ts.FAR) and np.array_equal(far.p.obs_uv, p.obs_uv)
    dbl = ts.variant(0, "double")
    assert dbl.p.points.shape[0] == 2 * p.points.shape[0] >= 66


@pytest.mark.parametrize("model", ts.MODELS)
def test_mu_iteration_settles_on_every_track(model):
    """A condition on the inputs: the restated device iteration settles within 24 rounds on every track of every cut.  Largest
    round count per model 0 .. 7: 5, 5, 5, 6, 5, 8, 6, 7.

    Under the kernel's FIRST rule alone (|dmu| <= 1e-13 mu) three tracks of these cuts never settle, in 200 rounds either: track 21
    of model 1 (7 views) and tracks 1 and 4 of model 6 (w = 0.25, on-axis).  Their mu is converged after three rounds and then
    alternates between two neighbouring values 1e-13 .. 3.2e-13 mu apart -- the rounding floor of a Rayleigh quotient of residuals
    of a pixel between numbers of 1e3 -- while their L2 vector is 1e-6 .. 1e-4 away from the SVD vector (bound 2e-10 .. 2e-9).  The
    kernel therefore also stops when the steps no longer shrink below 1e-10 mu; nview_svd_rounds restates both rules, and
    strict=True the first alone."""
    cut = ts.track_cut(model)
    worst, strict_unsettled = 0, []
    for t in range(cut.p.points.shape[0]):
        Ps, uv, _, sel = tr.track_inputs(cut.p, t)
        if len(sel) < 2:
            continue
        rounds, settled, x, _ = tr.nview_svd_rounds(Ps, uv)
        assert settled and rounds <= 24, (model, t, rounds)
        ref = tr.cut_references(model)[t]["svd"]
        if tr.eigen_tolerance(ref, tr.device_c("svd")) < COMPARABLE:
            assert tr.sign_error(x, ref["x"]) <= tr.eigen_tolerance(ref, tr.device_c("svd")), (model, t)
        worst = max(worst, rounds)
        if not tr.nview_svd_rounds(Ps, uv, strict=True)[1]:
            strict_unsettled.append(t)
    print("model %d: at most %d rounds; unsettled under the 1e-13 rule alone: %s" % (model, worst, strict_unsettled))
    assert worst <= 12


def test_search_for_an_unsettled_track():
    """400 two-view pinhole tracks 3 .. 3.6 degrees apart with 8 .. 50 px noise: every one settles, in 3 or 4 rounds (314 and 86
    of them), under either rule.  No input is known on which the iteration fails to settle, so the fall-back to the L2 vector
    stays unpinned; if this search ever finds one it belongs into the pinhole cut, next to the tracks built by hand."""
    found = []
    for seed, (cams, rays, X, uv) in enumerate(ts.two_view_candidates(400)):
        Ps = np.array([tr.projection_matrix(0, ts.HAND_CAMERA_K, e) for e in cams])
        assert tr.sufficient_angle(rays, ts.MIN_ANGLE_DEG)
        if not tr.nview_svd_rounds(Ps, uv)[1]:
            found.append(seed)
    assert not found, "the mu iteration does not settle on seeds %s: pin the fall-back on one of them" % found
