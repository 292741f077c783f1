"""GPU: theia_hip_filter_view_pairs_from_relative_translation and theia_hip_filter_view_pairs_from_orientation
(csrc/view_pair_filters.hip) against the numpy restatement (tests/translation_filter_ref.py), never against a second run
of the device code except where bit-identity of two runs is the point.

A scene is admitted to an equality test only if the restatement's own decisions are no near ties: every arg-max step's
best score at least 1e-9 (relative) above the second best, no pair's weight within 1e-9 (relative) of the threshold, no
squared residual within 1e-9 of the squared angle.  That is asserted of the restatement first; a scene that does not
meet it fails the test."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, ransac, sfm, twoview
from tests import filter_scenes as fs
from tests import rotation_scenes as rs
from tests import translation_filter_ref as ref

pytestmark = pytest.mark.gpu

INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
SWITCH = capi.MFAS_LDS_MAX_VIEWS

# name: (scene, num_iterations, tolerance)
SCENES = {
    "line": (lambda: fs.line_scene(), 48, 0.1),
    "ref_10_30_0": (lambda: fs.reference_translation_scene(10, 30, 0, seed=1), 48, 0.08),
    "ref_10_30_5": (lambda: fs.reference_translation_scene(10, 30, 5, seed=1), 48, 0.08),
    "ref_30_100_30": (lambda: fs.reference_translation_scene(30, 100, 30, seed=1), 48, 0.08),
    "v100_outliers": (lambda: fs.position_scene(100, 800, seed=1), 48, 0.08),
    "v60_isolated_three_components": (lambda: fs.components_scene(seed=2), 48, 0.08),
    "v63": (lambda: fs.position_scene(63, 400, seed=3), 48, 0.08),
    "v64": (lambda: fs.position_scene(64, 400, seed=4), 48, 0.08),
    "v65": (lambda: fs.position_scene(65, 400, seed=5), 48, 0.08),
    "v1023": (lambda: fs.position_scene(1023, 8000, seed=6), 48, 0.08),
    "v1025": (lambda: fs.position_scene(1025, 8000, seed=7), 48, 0.08),
    "v_switch_lds": (lambda: fs.position_scene(SWITCH, 30000, seed=8), 3, 0.08),
    "v_switch_global": (lambda: fs.position_scene(SWITCH + 1, 30000, seed=9), 3, 0.08),
    "v100_one_iteration": (lambda: fs.position_scene(100, 800, seed=10), 1, 0.08),
    "v2000_outliers": (lambda: fs.position_scene(2000, 30000, seed=1), 48, 0.08),
}
WANT = ("bad_weight", "order", "axes", "rotated")


def _options(iters, tol):
    o = global_pose.FilterViewPairsFromRelativeTranslationOptions()
    o.num_iterations, o.translation_projection_tolerance = iters, tol
    return o


def _device(s, iters, tol, **kw):
    rc, removed, out = global_pose.filter_translations_1dsfm(s["orientations"], s["pairs"], s["position_2"],
                                                             _options(iters, tol), want=WANT, **kw)
    assert rc == 0, capi.lib().theia_hip_last_error()
    return removed, out


def _admitted(r):
    assert r["min_gap"] >= 1e-9, r["min_gap"]
    assert r["threshold_margin"] >= 1e-9, r["threshold_margin"]


@pytest.mark.parametrize("name", list(SCENES))
def test_given_axes_match_the_restatement(name):
    make, iters, tol = SCENES[name]
    s = make()
    axes = fs.unit_axes(iters, seed=len(name))
    removed, out = _device(s, iters, tol, axes=axes)
    assert np.array_equal(out["axes"], axes)
    stats = global_pose.translation_filter_last_stats()
    assert stats["lds_route"] == (1 if s["n"] <= SWITCH else 0)
    # (6) the restatement on the device's rotated translations: the projections are then bit-equal, so the orders are
    # equal as integers and the weights are sums of the same terms
    r = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, tol, axes=axes,
                                rotated=out["rotated"])
    print(f"{name}: min gap {r['min_gap']:.3e}, threshold margin {r['threshold_margin']:.3e}, source steps "
          f"{r['source_steps']}, arg-max steps {r['argmax_steps']}, removed {int(r['removed'].sum())}")
    _admitted(r)
    assert np.array_equal(out["order"], r["order"])
    assert np.abs(out["bad_weight"] - r["bad_weight"]).max() <= 1e-13 * iters
    assert np.array_equal(removed, r["removed"])
    assert (stats["source_steps"], stats["argmax_steps"]) == (r["source_steps"], r["argmax_steps"])
    if "isolated" in s:
        assert len(s["isolated"]) == 6 and np.all(out["order"][:, s["isolated"]] == -1)
    # (7) the restatement on its own rotated translations (its own sin / cos)
    own = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, tol, axes=axes)
    _admitted(own)
    assert np.abs(out["rotated"] - own["rotated"]).max() <= 1e-14
    assert np.array_equal(out["order"], own["order"])
    assert np.array_equal(removed, own["removed"])


def test_switch_point_is_where_the_header_says():
    assert SWITCH == 5632
    assert set(SCENES) >= {"v_switch_lds", "v_switch_global"}


@pytest.mark.parametrize("name,seed", [("ref_30_100_30", 169), ("v100_outliers", 7), ("line", fs.LINE_SEED)])
def test_drawn_axes_and_generator_state(name, seed):
    make, iters, tol = SCENES[name]
    s = make()
    st = capi.RngState()
    L = ransac._sig()
    capi.check(L.theia_hip_rng_seed(C.byref(st), seed))
    removed, out = _device(s, iters, tol, rng_state=st)
    # the restatement's axes: the mirror's RandGaussian from the mean / variance of the device's rotated translations,
    # summed in pair order (the device sums in block order: 1e-12)
    rng = ransac.RandomNumberGenerator(seed)
    mean, var = ref.mean_variance(out["rotated"])
    axes = ref.draw_axes(mean, var, iters, rng.RandGaussian)
    assert np.abs(out["axes"] - axes).max() <= 1e-12
    assert np.abs(np.linalg.norm(out["axes"], axis=1) - 1.0).max() <= 1e-15
    mine = rng.thread_state()
    assert st.pos == mine.pos and st.mt[:] == mine.mt[:]            # left where exactly those draws end, word for word
    r = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, tol, axes=out["axes"],
                                rotated=out["rotated"])
    _admitted(r)
    assert np.array_equal(out["order"], r["order"]) and np.array_equal(removed, r["removed"])
    # a second call goes on from there
    _, out2 = _device(s, iters, tol, rng_state=st)
    axes2 = ref.draw_axes(mean, var, iters, rng.RandGaussian)
    assert np.abs(out2["axes"] - axes2).max() <= 1e-12
    assert not np.array_equal(out2["axes"], out["axes"])
    assert st.pos == rng.thread_state().pos and st.mt[:] == rng.thread_state().mt[:]


def test_two_runs_are_bit_identical():
    make, iters, tol = SCENES["v2000_outliers"]
    s = make()
    a, b = capi.RngState(), capi.RngState()
    for st in (a, b):
        capi.check(ransac._sig().theia_hip_rng_seed(C.byref(st), 11))
    r1, o1 = _device(s, iters, tol, rng_state=a)
    r2, o2 = _device(s, iters, tol, rng_state=b)
    assert np.array_equal(r1, r2)
    for k in WANT:
        assert o1[k].tobytes() == o2[k].tobytes(), k
    assert bytes(memoryview(a)) == bytes(memoryview(b))


def _view_pairs(s):
    vp = {}
    for k, (a, b) in enumerate(s["pairs"]):
        info = twoview.TwoViewInfo()
        info.position_2 = s["position_2"][k].copy()
        info.rotation_2 = s["rotation_2"][k].copy()
        vp[(int(a), int(b))] = info
    return vp, {v: s["orientations"][v].copy() for v in range(s["n"])}


@pytest.mark.parametrize("name,seed", [("line", fs.LINE_SEED), ("ref_30_100_30", 169)])
def test_pytheia_named_mirror(name, seed):
    make, iters, tol = SCENES[name]
    s = make()
    rng = ransac.RandomNumberGenerator(seed)
    r = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, tol, gauss=rng.RandGaussian)
    _admitted(r)
    gone = {tuple(int(v) for v in p) for p in s["pairs"][r["removed"]]}
    if name == "line":
        assert gone == {(0, 3)}
    for threads in (1, 8):
        vp, orient = _view_pairs(s)
        o = sfm.FilterViewPairsFromRelativeTranslationOptions()
        assert (o.num_threads, o.num_iterations, o.translation_projection_tolerance, o.rng) == (1, 48, 0.08, None)
        o.rng = ransac.RandomNumberGenerator(seed)
        o.num_threads = threads
        o.translation_projection_tolerance = tol
        n = sfm.FilterViewPairsFromRelativeTranslation(o, orient, vp)
        assert n == len(gone) and set(vp) == {tuple(int(v) for v in p) for p in s["pairs"]} - gone


def test_mirror_with_fewer_than_two_pairs_and_without_a_generator():
    s = fs.line_scene()
    vp, orient = _view_pairs(s)
    one = {(0, 3): vp[(0, 3)]}
    o = sfm.FilterViewPairsFromRelativeTranslationOptions()
    o.rng = ransac.RandomNumberGenerator(5)
    assert sfm.FilterViewPairsFromRelativeTranslation(o, orient, one) == 0 and list(one) == [(0, 3)]
    assert sfm.FilterViewPairsFromRelativeTranslation(o, orient, {}) == 0
    # the draws were still taken, 3 per iteration and call, as the reference takes them
    after = bytes(memoryview(o.rng.thread_state()))
    mine = ransac.RandomNumberGenerator(5)
    for _ in range(2 * 3 * 48):
        mine.RandGaussian(0.0, 1.0)
    assert bytes(memoryview(mine.thread_state())) == after
    o2 = sfm.FilterViewPairsFromRelativeTranslationOptions()   # rng = None: seeded from the clock, (0, 3) goes whatever the axes
    o2.translation_projection_tolerance = 0.1
    assert sfm.FilterViewPairsFromRelativeTranslation(o2, orient, vp) >= 1 and (0, 3) not in vp and (1, 2) in vp
    with pytest.raises(capi.TheiaHipError):
        vp2, orient2 = _view_pairs(s)
        del orient2[0]
        sfm.FilterViewPairsFromRelativeTranslation(o, orient2, vp2)


# name: (views, pairs, noise degrees, corrupted fraction, max degrees, view without orientation)
ORIENTATION_CASES = {
    "clean": (50, 300, 0.5, 0.0, 2.0, None),
    "corrupt_5": (50, 300, 0.5, 0.05, 2.0, None),
    "corrupt_30": (50, 300, 0.5, 0.3, 2.0, None),
    "missing_view": (50, 300, 0.5, 0.05, 2.0, 7),
    "deg_180": (50, 300, 0.5, 0.3, 180.0, 7),
    "deg_1e-3": (50, 300, 0.5, 0.0, 1e-3, None),
    "v3000": (3000, 40000, 1.0, 0.1, 1.5, 11),
}


@pytest.mark.parametrize("name", list(ORIENTATION_CASES))
def test_orientation_filter_matches_the_restatement(name):
    n, pairs, noise, corrupt, deg, missing = ORIENTATION_CASES[name]
    s = rs.make_scene(n, pairs, noise, corrupt, seed=len(name))
    has = None
    if missing is not None:
        has = np.ones(n, bool)
        has[missing] = False
    want, margin = ref.filter_orientations(s["edges"], s["gt"], s["rel"], deg, has)
    assert margin >= 1e-9, margin
    rc, got = global_pose.filter_pairs_from_orientation(s["gt"], s["edges"], s["rel"], deg, has)
    assert rc == 0, capi.lib().theia_hip_last_error()
    assert np.array_equal(got, want)
    names_missing = np.zeros(len(want), bool) if missing is None else (s["edges"] == missing).any(axis=1)
    if name == "deg_180":
        assert np.array_equal(got, names_missing) and names_missing.any()
    elif name == "deg_1e-3":
        assert got.all()
    else:
        assert np.array_equal(got, s["outliers"] | names_missing)   # 0.5 .. 1 degree of noise stays, a random rotation goes


def test_orientation_mirror_on_the_reference_scene():
    s = fs.reference_orientation_scene(10, 30, 15, seed=4)
    vp, orient = _view_pairs(s)
    assert sfm.FilterViewPairsFromOrientation(orient, 2.0, vp) == 15
    assert set(vp) == {tuple(int(v) for v in p) for p in s["pairs"][~s["invalid"]]}
    vp, orient = _view_pairs(s)
    del orient[3]
    n = sfm.FilterViewPairsFromOrientation(orient, 2.0, vp)
    gone = s["invalid"] | (s["pairs"] == 3).any(axis=1)
    assert n == int(gone.sum()) and set(vp) == {tuple(int(v) for v in p) for p in s["pairs"][~gone]}
    with pytest.raises(capi.TheiaHipError):
        sfm.FilterViewPairsFromOrientation(orient, -1.0, vp)


def _translation_call(n, pairs, aa, t, iters=48, tol=0.08, rng=True, axes=None):
    o = capi.TranslationFilterOptions()
    o.num_iterations, o.translation_projection_tolerance = iters, tol
    st = capi.RngState()
    capi.check(ransac._sig().theia_hip_rng_seed(C.byref(st), 3))
    before = bytes(memoryview(st))
    removed = np.full(len(pairs), 0x5A, dtype=np.uint8)
    weight = np.full(len(pairs), -7.0)
    rc = capi.lib().theia_hip_filter_view_pairs_from_relative_translation(
        n, len(pairs), capi.ptr(np.ascontiguousarray(pairs, dtype=np.int32), C.c_int32), capi.ptr(aa, C.c_double),
        capi.ptr(t, C.c_double), C.byref(o), C.byref(st) if rng else None, capi.ptr(axes, C.c_double),
        capi.ptr(removed, C.c_uint8), capi.ptr(weight, C.c_double), None, None, None)
    untouched = bool(np.all(removed == 0x5A) and np.all(weight == -7.0) and bytes(memoryview(st)) == before)
    return rc, untouched


def test_translation_filter_refusals():
    s = fs.reference_translation_scene(10, 30, 5, seed=1)
    n, p, aa, t = s["n"], s["pairs"].copy(), np.ascontiguousarray(s["orientations"]), np.ascontiguousarray(s["position_2"])
    assert _translation_call(n, p, aa, t) == (0, False)
    bad = p.copy(); bad[4, 1] = n
    assert _translation_call(n, bad, aa, t) == (INVALID, True)
    bad = p.copy(); bad[4, 0] = -1
    assert _translation_call(n, bad, aa, t) == (INVALID, True)
    bad = p.copy(); bad[4, 1] = bad[4, 0]
    assert _translation_call(n, bad, aa, t) == (INVALID, True)          # a self-pair
    bad = p.copy(); bad[20] = bad[3]
    assert _translation_call(n, bad, aa, t) == (INVALID, True)          # the same pair twice
    bad = p.copy(); bad[20] = bad[3][::-1]
    assert _translation_call(n, bad, aa, t) == (INVALID, True)          # ... and reversed: the same unordered pair
    assert _translation_call(n, p, aa, t, iters=0) == (INVALID, True)
    assert _translation_call(n, p, aa, t, iters=-3) == (INVALID, True)
    assert _translation_call(n, p, aa, t, tol=-0.01) == (INVALID, True)
    assert _translation_call(n, p, aa, t, tol=float("nan")) == (INVALID, True)
    assert _translation_call(n, p, aa, t, rng=False) == (INVALID, True)  # neither a generator nor axes
    assert _translation_call(n, p, aa, t, rng=False, axes=fs.unit_axes(48))[0] == 0
    # NULL options are the defaults
    st = capi.RngState()
    capi.check(ransac._sig().theia_hip_rng_seed(C.byref(st), 3))
    removed = np.zeros(len(p), dtype=np.uint8)
    axes = np.zeros((48, 3))
    rc = capi.lib().theia_hip_filter_view_pairs_from_relative_translation(
        n, len(p), capi.ptr(p, C.c_int32), capi.ptr(aa, C.c_double), capi.ptr(t, C.c_double), None, C.byref(st), None,
        capi.ptr(removed, C.c_uint8), None, None, capi.ptr(axes, C.c_double), None)
    assert rc == 0 and np.abs(np.linalg.norm(axes, axis=1) - 1.0).max() < 1e-15


def test_orientation_filter_refusals():
    s = fs.reference_orientation_scene(10, 30, 5, seed=4)
    aa, rel = np.ascontiguousarray(s["orientations"]), np.ascontiguousarray(s["rotation_2"])

    def call(pairs, deg):
        removed = np.full(len(pairs), 0x5A, dtype=np.uint8)
        rc = capi.lib().theia_hip_filter_view_pairs_from_orientation(
            s["n"], len(pairs), capi.ptr(np.ascontiguousarray(pairs, dtype=np.int32), C.c_int32), capi.ptr(aa, C.c_double),
            None, capi.ptr(rel, C.c_double), deg, capi.ptr(removed, C.c_uint8))
        return rc, bool(np.all(removed == 0x5A))

    p = s["pairs"]
    assert call(p, 2.0) == (0, False)
    assert call(p, -1e-9) == (INVALID, True)
    assert call(p, float("nan")) == (INVALID, True)
    bad = p.copy(); bad[2, 0] = 10
    assert call(bad, 2.0) == (INVALID, True)
    bad = p.copy(); bad[2, 0] = bad[2, 1]
    assert call(bad, 2.0) == (INVALID, True)
    bad = p.copy(); bad[9] = bad[1][::-1]
    assert call(bad, 2.0) == (INVALID, True)
