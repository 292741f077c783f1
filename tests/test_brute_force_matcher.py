"""CPU: the restatement the GPU tests of the brute-force matcher compare against (tests/brute_force_matcher_ref.py) on cases whose
answers can be read off, its float32 fma helper on a known answer, and the C-ABI's option defaults."""
import ctypes as C

import numpy as np

from pytheiasfm_amd import _capi as capi
from tests import brute_force_matcher_ref as ref

F32 = np.float32


def test_fmaf32_known_answer():
    """a b = 2^-24 (1 - 2^-46) lies just BELOW half an ulp of c = 1 + 2^-23, so the fused result is c; rounding a b + c to float64
    first lands exactly on the tie, which the second rounding takes to the even neighbour 1 + 2^-22."""
    a = F32(2.0 ** -24 * (1 + 2.0 ** -23)); b = F32(1 - 2.0 ** -23); c = F32(1 + 2.0 ** -23)
    assert float(a) == 2.0 ** -24 * (1 + 2.0 ** -23) and float(b) == 1 - 2.0 ** -23      # the inputs are float32 numbers
    assert ref.fmaf32(a, b, c) == F32(1 + 2.0 ** -23)
    assert ref.naive_fmaf32(a, b, c) == F32(1 + 2.0 ** -22)
    # elementwise on arrays, exact cases, and the sign of a cancelled sum
    x = np.array([3.0, -2.0, 0.0, 1.5], F32); y = np.array([2.0, 2.0, 0.0, 1.5], F32); z = np.array([1.0, 4.0, 0.0, -2.25], F32)
    got = ref.fmaf32(x, y, z)
    assert got.dtype == F32 and np.array_equal(got, np.array([7.0, 0.0, 0.0, 0.0], F32)) and not np.signbit(got).any()


def test_fmaf32_agrees_with_exact_rational_arithmetic():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(F32); b = rng.standard_normal(400).astype(F32)
    c = (-a.astype(np.float64) * b.astype(np.float64)).astype(F32) * F32(1 + 2.0 ** -12)   # heavy cancellation
    c[::2] = rng.standard_normal(200).astype(F32)
    got = ref.fmaf32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_three_by_three_matches_can_be_read_off():
    d1 = np.array([[0, 0], [10, 0], [0, 10]], F32); d2 = np.array([[0, 1], [10, 1], [0, 12]], F32)
    assert np.array_equal(ref.distance_matrix(d1, d2), np.array([[1, 101, 144], [101, 1, 244], [81, 181, 4]], F32))
    fd, fi, rd, ri = ref.knn2(d1, d2)
    assert fi.tolist() == [[0, 1], [1, 0], [2, 0]] and fd.tolist() == [[1, 101], [1, 101], [4, 81]]
    assert ri.tolist() == [[0, 2], [1, 0], [2, 0]] and rd.tolist() == [[1, 81], [1, 101], [4, 144]]
    want = [(0, 0, 1.0), (1, 1, 1.0), (2, 2, 4.0)]
    # min_num_feature_matches on both sides of the count
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=3) == (True, want)
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=4) == (False, [])
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, keep_only_symmetric_matches=False) == (True, want)
    # 4 < r^2 81 holds for r = 0.8 (51.84) and fails for r = 0.2 (3.24)
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, lowes_ratio=0.2) == (True, want[:2])


def test_duplicate_descriptor_fails_the_ratio_test():
    d1 = np.array([[1, 2]], F32); d2 = np.array([[5, 5], [1, 2], [1, 2]], F32)
    fd, fi, _, _ = ref.knn2(d1, d2)
    assert fd.tolist() == [[0, 0]] and fi.tolist() == [[1, 2]]              # clamped at 0, the lower index first
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, keep_only_symmetric_matches=False) == (True, [])   # 0 < r^2 0 is false
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, keep_only_symmetric_matches=False,
                                use_lowes_ratio=False) == (True, [(0, 1, 0.0)])


def test_tie_is_broken_by_index_in_both_directions():
    d1 = np.array([[0, 0]], F32); d2 = np.array([[0, 1], [1, 0], [-1, 0]], F32)
    fd, fi, rd, ri = ref.knn2(d1, d2)
    assert fd.tolist() == [[1, 1]] and fi.tolist() == [[0, 1]]
    assert ri.tolist() == [[0, -1]] * 3 and np.isinf(rd[:, 1]).all()          # one candidate: d1 = +inf, index -1
    fd, fi, rd, ri = ref.knn2(d2, d1)
    assert ri.tolist() == [[0, 1]] and rd.tolist() == [[1, 1]]
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, use_lowes_ratio=False) == (True, [(0, 0, 1.0)])
    # a side with one candidate passes the ratio test, a side with none yields nothing
    assert ref.match_image_pair(d2[:1], d1, min_num_feature_matches=0) == (True, [(0, 0, 1.0)])
    assert ref.match_image_pair(d1, np.zeros((0, 2), F32), min_num_feature_matches=0) == (True, [])
    assert ref.match_image_pair(np.zeros((0, 2), F32), d2, min_num_feature_matches=0) == (True, [])


def test_forward_match_dropped_by_the_symmetric_test():
    d1 = np.array([[0, 0], [1, 0]], F32); d2 = np.array([[1.25, 0], [50, 0]], F32)
    fwd = [(0, 0, 1.5625), (1, 0, 0.0625)]
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0, keep_only_symmetric_matches=False) == (True, fwd)
    # image 2's feature 0 answers feature 1; its feature 1 fails the ratio test (2401 against 2500)
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=0) == (True, fwd[1:])
    # the early return on the forward count and the final count
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=2, keep_only_symmetric_matches=False) == (True, fwd)
    assert ref.match_image_pair(d1, d2, min_num_feature_matches=2) == (False, [])


def margin_scene(seed=7, ntrue=150, nextra=60, dim=128, noise=0.02):
    rng = np.random.default_rng(seed)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    base = unit(rng.standard_normal((ntrue, dim)))
    d1 = np.concatenate([unit(base + noise * rng.standard_normal((ntrue, dim))), unit(rng.standard_normal((nextra, dim)))])
    d2 = np.concatenate([unit(base + noise * rng.standard_normal((ntrue, dim))), unit(rng.standard_normal((nextra, dim)))])
    perm = rng.permutation(len(d2))
    truth = {i: int(np.argsort(perm)[i]) for i in range(ntrue)}
    return d1, np.ascontiguousarray(d2[perm]), truth


def test_expansion_changes_no_decision_on_a_margin_scene():
    """150 true pairs + 60 distractors per image, unit norm, dim 128, noise 0.02: a true pair lies at d ~ 2 * 128 * 0.02^2 = 0.1,
    everything else at d ~ 2, so every decision has a margin far above the expansion's rounding error (~1e-6)."""
    d1, d2, truth = margin_scene()
    ok, got = ref.match_image_pair(d1, d2)
    ok64, want = ref.direct_f64_matches(d1, d2)
    assert ok and ok64
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert {a: b for a, b, _ in got} == truth
    assert max(abs(float(x[2]) - float(y[2])) for x, y in zip(got, want)) < 1e-5


def test_option_defaults_match_the_reference_struct():
    o = capi.BruteForceOptions()
    assert C.sizeof(o) == 5 * 4
    capi.lib().theia_hip_brute_force_options_default(C.byref(o))
    # feature_matcher_options.h:66-87
    assert o.keep_only_symmetric_matches == 1 and o.use_lowes_ratio == 1 and o.lowes_ratio == np.float32(0.8)
    assert o.min_num_feature_matches == 30 and o.max_pairs_per_launch == 0
    from pytheiasfm_amd import matching
    m = matching.FeatureMatcherOptions()
    c = m.to_c()
    assert (m.keep_only_symmetric_matches, m.use_lowes_ratio, m.perform_geometric_verification) == (True, True, True)
    assert c.lowes_ratio == np.float32(0.8) and c.min_num_feature_matches == 30
