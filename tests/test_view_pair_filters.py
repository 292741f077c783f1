"""CPU: RandGaussian against the real libstdc++ (stored draws and generator positions), and the numpy restatement of the
two view-graph filters (tests/translation_filter_ref.py) on the reference's own test scenes
(filter_view_pairs_from_relative_translation_test.cc, filter_view_pairs_from_orientation_test.cc), which pins the
restatement the GPU tests compare the device against."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ransac
from tests import filter_scenes as fs
from tests import translation_filter_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

def test_rand_gaussian_matches_libstdcxx_golden():
    rows = json.load(open(os.path.join(HERE, "golden", "mt19937_randgaussian.json")))["randgaussian"]
    assert len(rows) == 1000
    assert any(r[2] == 0.0 for r in rows) and any(r[1] < 0.0 for r in rows)   # std_dev = 0 and a negative mean are in
    for seed in sorted({r[0] for r in rows}):
        rng = ransac.RandomNumberGenerator(seed)
        reference_words = np.random.RandomState(seed)   # the same MT19937: the state after `words` raw outputs
        taken = 0
        for _, mean, std_dev, value, pos, words in (r for r in rows if r[0] == seed):
            assert rng.RandGaussian(mean, std_dev) == value
            assert rng.thread_state().pos == pos
            reference_words.randint(0, 2 ** 32, size=words - taken, dtype=np.uint64)
            taken = words
            key, p = reference_words.get_state(legacy=True)[1:3]
            assert p == pos and np.array_equal(np.array(rng.thread_state().mt[:], dtype=np.uint32), key)


def test_rand_gaussian_batch_equals_single_draws_and_refuses_bad_arguments():
    L = ransac._sig()
    a, b = capi.RngState(), capi.RngState()
    capi.check(L.theia_hip_rng_seed(C.byref(a), 31))
    capi.check(L.theia_hip_rng_seed(C.byref(b), 31))
    out = np.zeros(9)
    capi.check(L.theia_hip_rng_rand_gaussian(C.byref(a), -0.5, 0.25, 9, capi.ptr(out, C.c_double)))
    one = C.c_double(0.0)
    for k in range(9):
        capi.check(L.theia_hip_rng_rand_gaussian(C.byref(b), -0.5, 0.25, 1, C.byref(one)))
        assert one.value == out[k]
    assert bytes(memoryview(a)) == bytes(memoryview(b))
    before = bytes(memoryview(a))
    assert L.theia_hip_rng_rand_gaussian(None, 0.0, 1.0, 1, capi.ptr(out, C.c_double)) != 0
    assert L.theia_hip_rng_rand_gaussian(C.byref(a), 0.0, 1.0, -1, capi.ptr(out, C.c_double)) != 0
    assert L.theia_hip_rng_rand_gaussian(C.byref(a), 0.0, 1.0, 2, None) != 0
    assert bytes(memoryview(a)) == before
    a.pos = 625
    assert L.theia_hip_rng_rand_gaussian(C.byref(a), 0.0, 1.0, 1, capi.ptr(out, C.c_double)) != 0


def _filter(scene, seed, **kw):
    rng = ransac.RandomNumberGenerator(seed)
    return ref.filter_translations(scene["n"], scene["pairs"], scene["orientations"], scene["position_2"],
                                   gauss=rng.RandGaussian, **kw)


@pytest.mark.parametrize("views,valid,invalid", [(10, 30, 0), (10, 30, 5), (30, 100, 30)])
def test_restatement_keeps_the_valid_pairs_of_the_reference_scenes(views, valid, invalid):
    s = fs.reference_translation_scene(views, valid, invalid, seed=1)
    r = _filter(s, 169)
    assert len(s["pairs"]) == valid + invalid
    assert len(s["pairs"]) - int(r["removed"].sum()) >= valid        # EXPECT_GE(view_graph.NumEdges(), num_valid_view_pairs)
    assert r["source_steps"] + r["argmax_steps"] == 48 * views
    for o in r["order"]:
        assert sorted(o.tolist()) == list(range(views))              # every view is taken exactly once


def test_restatement_line_test():
    s = fs.line_scene()
    r = _filter(s, fs.LINE_SEED, tolerance=0.1)
    assert r["removed"].tolist() == [False, False, False, True]       # EXPECT_EQ(view_graph.NumEdges(), kValidViewPairs)
    # Whatever the axes: with a = the axis' x component (the projection of the three chain pairs) and b = the projection
    # of (0, 3), the four views form a cycle exactly when a and b differ in sign, and then all have one incoming pair, so
    # the arg-max takes view 0 or view 3 first (scores (|b| + 1) / (|a| + 1) and its inverse; views 1 and 2 score 1):
    #   a > 0 > b:  |a| > |b|: order 0 1 2 3, (0, 3) is bad by |b|;   |b| > |a|: order 3 0 1 2, (2, 3) is bad by |a|
    #   a < 0 < b:  |b| > |a|: order 0 3 2 1, (0, 1) is bad by |a|;   |a| > |b|: order 3 2 1 0, (0, 3) is bad by |b|
    # so (1, 2) never collects weight, (0, 3) collects most of it, and which chain pair collects the rest depends on the
    # axes.  The restatement must give exactly these sums.
    some_on_01 = some_on_23 = False
    for seed in range(180, 212):
        r = _filter(s, seed, tolerance=0.1)
        want = np.zeros(4)
        for axis in r["axes"]:
            a, b = ref.project(r["rotated"], axis)[[0, 3]]
            if a * b < 0.0:
                assert abs(abs(a) - abs(b)) > 1e-9 * abs(a)              # no near tie decides an order
                first = 0 if (abs(a) > abs(b)) == (a > 0.0) else 3
                bad = 3 if (first == 0) == (a > 0.0) else (2 if a > 0.0 else 0)
                want[bad] += abs(b) if bad == 3 else abs(a)
        assert np.abs(r["bad_weight"] - want).max() <= 1e-12
        assert r["bad_weight"][1] == 0.0
        assert r["removed"][3] and not r["removed"][1]
        some_on_01 |= bool(r["bad_weight"][0] > 0.0)
        some_on_23 |= bool(r["bad_weight"][2] > 0.0)
    assert some_on_01 and some_on_23


@pytest.mark.parametrize("views,valid,invalid", [(10, 30, 5), (30, 100, 30), (200, 3000, 300)])
def test_choice_among_sources_does_not_change_the_weights(views, valid, invalid):
    s = fs.reference_translation_scene(views, valid, invalid, seed=2)
    iters = 12 if views > 100 else 48
    axes = fs.unit_axes(iters, seed=views)
    low = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, axes=axes)
    pick = np.random.default_rng(5).choice
    rnd = ref.filter_translations(s["n"], s["pairs"], s["orientations"], s["position_2"], iters, axes=axes, rule="random",
                                  pick=pick)
    assert low["argmax_steps"] > 0
    assert not np.array_equal(low["order"], rnd["order"])             # the order numbers do change ...
    assert np.array_equal(low["bad_weight"], rnd["bad_weight"])       # ... the weights do not, not by a bit
    assert np.array_equal(low["removed"], rnd["removed"])


def test_fewer_than_two_pairs_remove_nothing():
    s = fs.line_scene()
    r = ref.filter_translations(4, s["pairs"][3:], s["orientations"], s["position_2"][3:], gauss=lambda m, sd: 0.0)
    assert r["removed"].tolist() == [False] and np.isnan(r["axes"]).all()
    mean, var = ref.mean_variance(s["position_2"][3:])
    assert np.isnan(var).all()                                        # 0 / 0: the reference's NaN axis


def test_rotation_restatement_matches_the_rotation_matrix():
    from tests.rotation_averaging_ref import aa_to_R
    s = fs.reference_translation_scene(30, 100, 30, seed=3)
    got = ref.rotate_translations(s["orientations"], s["pairs"], s["position_2"])
    want = np.einsum("eji,ej->ei", aa_to_R(s["orientations"][s["pairs"][:, 0]]), s["position_2"])   # R_1' t
    assert np.abs(got - want).max() < 1e-14
    valid = ~s["invalid"]
    d = s["positions"][s["pairs"][:, 1]] - s["positions"][s["pairs"][:, 0]]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.abs(got[valid] - d[valid]).max() < 1e-14                # a valid pair's direction in the global frame


@pytest.mark.parametrize("views,valid,invalid", [(10, 30, 0), (10, 30, 5), (10, 30, 15)])
def test_orientation_restatement_on_the_reference_scenes(views, valid, invalid):
    s = fs.reference_orientation_scene(views, valid, invalid, seed=4)
    removed, margin = ref.filter_orientations(s["pairs"], s["orientations"], s["rotation_2"], 2.0)
    assert len(s["pairs"]) == valid + invalid
    assert np.array_equal(removed, s["invalid"])                      # EXPECT_EQ(view_graph.NumEdges(), num_valid_view_pairs)
    assert margin > 1e-9
    has = np.ones(views, bool)
    has[3] = False
    removed2, _ = ref.filter_orientations(s["pairs"], s["orientations"], s["rotation_2"], 2.0, has)
    assert np.array_equal(removed2, s["invalid"] | (s["pairs"] == 3).any(axis=1))


def test_new_symbols_are_listed():
    for name in ("theia_hip_filter_view_pairs_from_relative_translation", "theia_hip_filter_view_pairs_from_orientation",
                 "theia_hip_translation_filter_last_stats", "theia_hip_rng_rand_gaussian"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)
    header = open(os.path.join(os.path.dirname(HERE), "include", "theia_hip.h")).read()
    assert f"#define THEIA_MFAS_LDS_MAX_VIEWS {capi.MFAS_LDS_MAX_VIEWS}\n" in header
    assert C.sizeof(capi.TranslationFilterOptions) == 16 and C.sizeof(capi.TranslationFilterStats) == 5 * 8 + 2 * 8 + 2 * 4
