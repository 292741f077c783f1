"""GPU tests of the Sim(3) alignment: theia_hip_sim3_maps, theia_hip_optimize_alignment_sim3 (both routes) and the mirror in
pytheiasfm_amd/alignment.py, against tests/sim3_ref.py (numpy maps, jacfwd Jacobians, Ceres' loop) and
tests/golden/sim3_maps.npz.

SCENES.  The reference's GenerateSyntheticPointCloud(n, 0.01) (align_point_clouds_test.cc:204-220; the noise from numpy's
default_rng(SEED), SEED = 5) mapped by its ground truth (translation (1, 2, 0.5), rotation (0.1, 0.05, 0.02), scale 1.5),
every problem from the reference's as-written start (0,0,0,0,0,0,1).  For SEED = 5 the comparator's float64 and longdouble
runs agree on the termination and on every count of every problem (checked on the CPU by test_seed_is_stable below, which
needs no GPU but lives here with the scenes); so does the run on coordinates moved by one ulp (below).

TOLERANCE OF THE SOLVES.  The comparator sums the points in index order, the device in lane / butterfly / wave order; equality
is not expected.  The comparator runs with float64 and with longdouble sums; the spread between the two runs is the
yardstick and the device is allowed 10 x it, on every row of the cost trace and on the parameters.  That spread sees the
order of the sums only.  The device also differs from numpy in libm's last bits and in the order of operations inside exp
and the residual, and with n = 1 or 2 (one term per lane, no sum to reorder) the spread is exactly zero while the damped,
rank-deficient systems of those problems amplify any rounding (measured on the device: 5e-13 on a cost of 41 at n = 1).
So a third run moves every coordinate of source and target by one unit in the last place (random signs) and the yardstick
is the larger of the two spreads -- still the comparator's own sensitivity to rounding, never the device's result.
Measured on the MI355X over all problems of this file: the device's largest deviation is 2.2 x the yardstick on the costs
and 1.8 x on the parameters (10 x allowed); no count differed, so nothing was excused.  Measured spreads on these
scenes: costs 0 .. 2e-9 (absolute, largest row; the costs start near 0.5 n 100), parameters 0 .. 2e-9 (point-to-plane with
constant normals is ill-conditioned; the others stay below 1e-15).  The spread can be zero (n = 1, 2: one term per sum) or
small by chance (3e-15 at n = 1000, where another order of the same float64 sum moves the cost by 6e-13), so it is floored at
one rounding of the numbers summed: 2^-52 x the largest cost of the trace, and 2^-52 x max(1, largest parameter).
Iteration counts must agree; a problem may be excused only if the comparator's last accepted relative cost change lies
within 10 x of the function tolerance, and at most 1 problem in 10 may be.

TOLERANCE OF THE MAPS: as tests/test_sim3_alignment.py states it -- 4 x the numpy restatement's own error per calcW branch."""
import ctypes as C
import functools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import alignment as al
from tests import sim3_ref as ref
from tests import test_sim3_alignment as cpu

SEED = 5
EPS64 = 2.0 ** -52
START = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
GT = ref.create_sim3([1.0, 2.0, 0.5], [0.1, 0.05, 0.02], 1.5)
COUNTS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000]
KINDS = [ref.POINT_TO_POINT, ref.ROBUST_POINT_TO_POINT, ref.POINT_TO_PLANE]
HUBER = 0.5


class Case:
    def __init__(self, n, kind, rng, weights=False, normals=True, start=START, max_iterations=100):
        self.n, self.kind = n, kind
        self.src = ref.synthetic_cloud(n, 0.01, rng) if n else np.zeros((0, 3))
        self.tgt = ref.transform_cloud(self.src, GT) if n else np.zeros((0, 3))
        self.w = rng.uniform(0.5, 2.0, size=n) if weights else np.ones(n)
        self.nrm = np.tile([0.0, 0.0, 2.0], (n, 1)) if normals else None   # not unit: the functor normalises
        self.start, self.max_iterations = np.array(start, dtype=np.float64), max_iterations
        # what the comparator may not be held to: fewer points than unknowns, or constant normals (z only)
        self.underdetermined = n < 3 or (kind == ref.POINT_TO_PLANE and normals)

    def problem(self):
        return ref.Problem(self.src, self.tgt, self.kind, weights=self.w, normals=self.nrm, huber_threshold=HUBER)

    def options(self):
        o = al.Sim3AlignmentOptions()
        o.alignment_type, o.huber_threshold, o.max_iterations = self.kind, HUBER, self.max_iterations
        return o


@functools.lru_cache(maxsize=None)
def group_cases():
    rng = np.random.default_rng(SEED)
    cases = [Case(n, k, rng) for k in KINDS for n in COUNTS]
    cases.insert(len(cases) // 2, Case(0, ref.POINT_TO_POINT, rng))       # no points, in the middle
    cases.append(Case(100, ref.POINT_TO_POINT, rng, weights=True))         # per-point weights
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def expected(case):
    """the comparator's runs, once per case: float64 sums, longdouble sums, and float64 sums on coordinates moved by one
    unit in the last place (module docstring)"""
    rng = np.random.default_rng(SEED + 1000 + case.n)
    moved = case.problem()
    moved.x = moved.x * (1.0 + EPS64 * rng.choice([-1.0, 1.0], size=moved.x.shape))
    moved.y = moved.y * (1.0 + EPS64 * rng.choice([-1.0, 1.0], size=moved.y.shape))
    return (ref.solve(case.problem(), case.start, case.max_iterations, np.float64),
            ref.solve(case.problem(), case.start, case.max_iterations, np.longdouble),
            ref.solve(moved, case.start, case.max_iterations, np.float64))


def _counts(r):
    return (r.termination, r.num_iterations, r.successful, r.unsuccessful, r.invalid)


def run_device(cases, with_normals=True, want_trace=True):
    return al.optimize_alignment_sim3([c.src for c in cases], [c.tgt for c in cases], [c.start for c in cases],
                                      [c.options() for c in cases], weights=[c.w for c in cases],
                                      normals=[c.nrm if c.nrm is not None else np.tile([0.0, 0.0, 1.0], (c.n, 1)) for c in cases]
                                      if with_normals else None, want_trace=want_trace)


def compare(case, params, summ, trace, excuses):
    """one problem against the comparator under the module docstring's rule; appends to `excuses` when the counts differ
    and the rule allows it"""
    a, b, c = expected(case)
    assert summ.success == int(a.success)
    if case.n == 0:
        assert summ.termination == capi.THEIA_SIM3_TERM_NO_POINTS and np.array_equal(params, case.start)
        assert summ.num_iterations == 0 and summ.final_cost == 0.0 and summ.alignment_error == 0.0
        return
    counts = (summ.termination, summ.num_iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_invalid_steps)
    want = _counts(a)
    rows = min(len(trace), len(a.trace))
    ta, tb, tc = (np.array(r.trace)[:rows, 0] for r in (a, b, c))
    if counts != want:
        near = a.last_rel_change <= 10.0 * 1e-6
        print(f"n {case.n} kind {case.kind}: counts {counts} comparator {want} last relative change {a.last_rel_change:.2e}")
        assert near, (case.n, case.kind, counts, want, a.last_rel_change)
        excuses.append((case.n, case.kind))
        rows -= 1                                                         # the runs part ways in their last row
    else:
        assert len(trace) == len(a.trace) and np.array_equal(trace[:, 4], np.array(a.trace)[:, 4])
    yard = max(np.abs(ta - tb).max(), np.abs(ta - tc).max(), EPS64 * np.abs(ta).max())
    got = np.abs(trace[:rows, 0] - ta[:rows]).max()
    print(f"n {case.n} kind {case.kind}: counts {counts} cost yardstick {yard:.2e} device {got:.2e}", end="")
    assert got <= 10.0 * yard, (case.n, case.kind, got, yard)
    if counts == want:
        assert abs(summ.final_cost - a.final_cost) <= 10.0 * yard and abs(summ.initial_cost - a.initial_cost) <= 10.0 * yard
    if not case.underdetermined and counts == want:
        yp = max(np.abs(a.params - b.params).max(), np.abs(a.params - c.params).max(), EPS64 * max(1.0, np.abs(a.params).max()))
        gp = np.abs(params - a.params).max()
        print(f" | parameter yardstick {yp:.2e} device {gp:.2e}", end="")
        assert gp <= 10.0 * yp, (case.n, case.kind, gp, yp)
        assert abs(summ.alignment_error - a.alignment_error) <= 1e-9      # a mean of distances of unit size
    print()


def test_seed_is_stable():
    """no GPU: for SEED the comparator's three runs agree on every count (module docstring)"""
    for case in group_cases() + grid_cases():
        a, b, c = expected(case)
        assert _counts(a) == _counts(b) == _counts(c), (case.n, case.kind)
        assert len(a.trace) == len(b.trace) == len(c.trace)


@pytest.mark.gpu
def test_maps_on_device_against_golden():
    tol_e, tol_l, _, _ = cpu.map_tolerances()
    g = cpu.GOLDEN
    E = al.sim3_maps(capi.THEIA_SIM3_MAP_EXP, cpu.TANGENTS)
    L = al.sim3_maps(capi.THEIA_SIM3_MAP_LOG, g["log_in"])
    li = g["log_in"]
    F = al.sim3_maps(capi.THEIA_SIM3_MAP_FROM_RTS, np.concatenate([li[:, 1:13], li[:, :1]], axis=1))
    T = al.sim3_maps(capi.THEIA_SIM3_MAP_TO_RTS, cpu.TANGENTS)
    M = al.sim3_maps(capi.THEIA_SIM3_MAP_TO_MATRIX4, cpu.TANGENTS)
    got_e, got_l = cpu.branch_errors(E, g["exp_hi"]), cpu.branch_errors(L, g["log_hi"])
    for b in sorted(got_e):
        print(f"branch {b}: exp device {got_e[b]:.2e} allowed {tol_e[b]:.2e} | log device {got_l[b]:.2e} allowed {tol_l[b]:.2e}")
        assert got_e[b] <= tol_e[b] and got_l[b] <= tol_l[b]
    assert np.array_equal(F, L)
    for i, b in enumerate(cpu.BRANCHES):
        assert np.array_equal(M[i].reshape(4, 4)[:3, :3].reshape(-1), E[i][:9]) and np.array_equal(M[i].reshape(4, 4)[:3, 3], E[i][9:])
        assert np.array_equal(M[i][12:], [0.0, 0.0, 0.0, 1.0])
        assert cpu.rel_err(T[i][9:12], g["exp_hi"][i][9:12]) <= tol_e[b]
        assert abs(T[i][12] - li[i][0]) <= 4.0 * EPS64 * li[i][0]
        assert np.abs(T[i][:9] - li[i][1:10]).max() <= 16.0 * EPS64


@pytest.mark.gpu
def test_group_route_batch_against_comparator():
    cases = group_cases()
    params, summ, traces = run_device(cases)
    excuses = []
    for c, p, s, t in zip(cases, params, summ, traces):
        assert s.route == 0
        compare(c, p, s, t, excuses)
    assert len(excuses) * 10 <= len(cases), excuses


@pytest.mark.gpu
def test_plane_without_normals_is_point_to_point():
    rng = np.random.default_rng(SEED + 1)
    cases = [Case(65, ref.POINT_TO_PLANE, rng, normals=False), Case(65, ref.POINT_TO_POINT, rng)]
    cases[1].src, cases[1].tgt = cases[0].src, cases[0].tgt
    params, summ, traces = run_device(cases, with_normals=False)
    compare(cases[0], params[0], summ[0], traces[0], [])
    assert params[0].tobytes() == params[1].tobytes() and traces[0].tobytes() == traces[1].tobytes()


@pytest.mark.gpu
def test_output_bytes_do_not_depend_on_the_batch_or_the_run():
    cases = group_cases()
    k = next(i for i, c in enumerate(cases) if c.n == 257 and c.kind == ref.ROBUST_POINT_TO_POINT)
    one = cases[k]
    outs = [run_device([one]), run_device([one]), run_device(list(cases[:4]) + [one]), run_device([one] + list(cases[-3:]))]
    where = [0, 0, 4, 0]
    blobs = [(o[0][i].tobytes(), bytes(o[1][i]), o[2][i].tobytes()) for o, i in zip(outs, where)]
    assert all(b == blobs[0] for b in blobs[1:])


@functools.lru_cache(maxsize=None)
def grid_cases():
    rng = np.random.default_rng(SEED + 2)
    return tuple(Case(257, k, rng) for k in KINDS) + (Case(257, ref.POINT_TO_POINT, rng, weights=True),)


@pytest.mark.gpu
def test_grid_route_by_override(monkeypatch):
    """a 257-point problem sent down the grid route (two workgroups) by the internal override"""
    monkeypatch.setenv("THEIA_HIP_SIM3_GROUP_MAX_POINTS", "256")
    cases = grid_cases()
    first = run_device(cases)
    second = run_device(cases)
    excuses = []
    for i, c in enumerate(cases):
        assert first[1][i].route == 1
        compare(c, first[0][i], first[1][i], first[2][i], excuses)
        assert first[0][i].tobytes() == second[0][i].tobytes() and bytes(first[1][i]) == bytes(second[1][i])
        assert first[2][i].tobytes() == second[2][i].tobytes()
    assert not excuses
    monkeypatch.delenv("THEIA_HIP_SIM3_GROUP_MAX_POINTS")
    group = run_device(cases)                                              # the same problems in one workgroup each
    for i, c in enumerate(cases):
        assert group[1][i].route == 0
        compare(c, group[0][i], group[1][i], group[2][i], excuses)


@pytest.mark.gpu
def test_grid_route_above_the_threshold():
    """one problem of THEIA_SIM3_GROUP_MAX_POINTS + 1 points: the grid route without the override"""
    rng = np.random.default_rng(SEED + 3)
    c = Case(capi.THEIA_SIM3_GROUP_MAX_POINTS + 1, ref.POINT_TO_POINT, rng)
    first, second = run_device([c]), run_device([c])
    assert first[1][0].route == 1
    compare(c, first[0][0], first[1][0], first[2][0], [])
    assert first[0].tobytes() == second[0].tobytes() and bytes(first[1][0]) == bytes(second[1][0])
    assert first[2][0].tobytes() == second[2][0].tobytes()


@pytest.mark.gpu
def test_robust_outlier_scene():
    """the reference's outlier scene (:297-343): 5 of 100 targets shifted by (2, 2, 2), Huber 0.5"""
    rng = np.random.default_rng(SEED + 4)
    c = Case(100, ref.ROBUST_POINT_TO_POINT, rng)
    c.tgt = c.tgt.copy()
    c.tgt[:5] += [2.0, 2.0, 2.0]
    params, summ, traces = run_device([c])
    compare(c, params[0], summ[0], traces[0], [])
    assert summ[0].success == 1 and summ[0].alignment_error < 5.0
    assert ref.Problem(c.src, c.tgt).alignment_error(params[0]) < 5.0


@pytest.mark.gpu
def test_terminations():
    rng = np.random.default_rng(SEED + 5)
    one = Case(100, ref.POINT_TO_POINT, rng, max_iterations=1)
    at_optimum = Case(100, ref.POINT_TO_POINT, rng, start=GT)
    at_optimum.src = ref.synthetic_cloud(100, 0.0)
    at_optimum.tgt = ref.transform_cloud(at_optimum.src, GT)
    params, summ, traces = run_device([one, at_optimum])
    assert summ[0].termination == capi.THEIA_SIM3_TERM_MAX_ITERATIONS and summ[0].success == 0 and summ[0].num_iterations == 2
    compare(one, params[0], summ[0], traces[0], [])
    assert summ[1].termination == capi.THEIA_SIM3_TERM_GRADIENT_TOLERANCE and summ[1].success == 1 and summ[1].num_iterations == 1
    assert np.array_equal(params[1], GT)


def _raw_call(offsets, src, tgt, start, opts, weights=None, normals=None, null=()):
    """the C entry with sentinel-filled outputs -> (return code, params, summary bytes)"""
    P = len(offsets) - 1
    offsets = np.asarray(offsets, dtype=np.int64)
    params = np.full((max(P, 1), 7), -7.5)
    summ = (capi.Sim3AlignmentSummaryC * max(P, 1))()
    C.memset(summ, 0x5A, C.sizeof(summ))
    copt = (capi.Sim3AlignmentOptionsC * max(P, 1))()
    for i, (kind, iters, huber, pw) in enumerate(opts):
        copt[i].alignment_type, copt[i].max_iterations, copt[i].huber_threshold, copt[i].point_weight = kind, iters, huber, pw
    arg = dict(offsets=capi.ptr(offsets, C.c_int64), source=capi.ptr(src, C.c_double), target=capi.ptr(tgt, C.c_double),
               weights=capi.ptr(weights, C.c_double), normals=capi.ptr(normals, C.c_double), start=capi.ptr(start, C.c_double),
               options=copt, params=capi.ptr(params, C.c_double), summary=summ)
    for k in null:
        arg[k] = None
    rc = capi.lib().theia_hip_optimize_alignment_sim3(P if "count" not in null else -1, arg["offsets"], arg["source"], arg["target"],
                                                      arg["weights"], arg["normals"], arg["start"], arg["options"], arg["params"],
                                                      arg["summary"], None, 0, None)
    return rc, params, bytes(summ)


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    rng = np.random.default_rng(SEED + 6)
    n = 10
    src = np.ascontiguousarray(ref.synthetic_cloud(n, 0.01, rng))
    tgt = np.ascontiguousarray(ref.transform_cloud(src, GT))
    ones, nrm, start = np.ones(n), np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (n, 1))), START.copy().reshape(1, 7)
    ok = [(0, 100, 0.5, 1.0)]

    def bad(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b
    refused = {
        "null source": dict(null=("source",)), "null target": dict(null=("target",)), "null start": dict(null=("start",)),
        "null offsets": dict(null=("offsets",)), "null options": dict(null=("options",)), "null params": dict(null=("params",)),
        "null summary": dict(null=("summary",)), "negative count": dict(null=("count",)),
        "descending offsets": dict(offsets=[0, 6, 4], opts=ok * 2, start=np.tile(START, (2, 1))),
        "nan source": dict(src=bad(src, 4, np.nan)), "inf target": dict(tgt=bad(tgt, 5, np.inf)),
        "nan weight": dict(weights=bad(ones, 3, np.nan)), "inf start": dict(start=bad(start, 6, np.inf)),
        "nan normal": dict(normals=bad(nrm, 2, np.nan), opts=[(2, 100, 0.5, 1.0)]),
        "zero normal": dict(normals=bad(nrm, 5, 0.0), opts=[(2, 100, 0.5, 1.0)]),
        "negative max_iterations": dict(opts=[(0, -1, 0.5, 1.0)]),
        "zero huber": dict(opts=[(1, 100, 0.0, 1.0)]), "negative huber": dict(opts=[(1, 100, -1.0, 1.0)]),
        "unknown type": dict(opts=[(3, 100, 0.5, 1.0)]),
    }
    base = dict(offsets=[0, n], src=src, tgt=tgt, start=start, opts=ok)
    for name, change in refused.items():
        rc, params, sb = _raw_call(**{**base, **change})
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, name
        assert np.all(params == -7.5) and sb == b"\x5a" * len(sb), name
    rc, params, sb = _raw_call(**base)                                    # and the same call, unchanged, is accepted
    assert rc == 0 and not np.any(params == -7.5)
    rc = capi.lib().theia_hip_sim3_maps(9, 1, capi.ptr(START.copy(), C.c_double), capi.ptr(np.zeros(16), C.c_double))
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_mirror():
    rng = np.random.default_rng(SEED + 7)
    src = ref.synthetic_cloud(100, 0.01, rng)
    tgt = ref.transform_cloud(src, GT)
    prob = ref.Problem(src, tgt)
    # as written: the solve starts at (0,0,0,0,0,0,1) whatever the options say
    s = al.OptimizeAlignmentSim3(src, tgt)
    a = ref.solve(prob, START, 100)
    assert s.success and s.num_iterations == a.num_iterations and np.abs(s.sim3_params - a.params).max() < 1e-12
    o = al.Sim3AlignmentOptions()
    o.set_initial_sim3_params(ref.create_sim3([0.5, 1.0, 0.2], [0.05, 0.02, 0.01], 1.2))
    s2 = al.OptimizeAlignmentSim3(src, tgt, o)
    assert s2.sim3_params.tobytes() == s.sim3_params.tobytes() and s2.num_iterations == s.num_iterations
    # as the comments intend: from the Umeyama result
    o = al.Sim3AlignmentOptions()
    o.perform_optimization = False
    init = al.OptimizeAlignmentSim3(src, tgt, o)
    R, t, sc = al.AlignPointCloudsUmeyamaWithWeights(src, tgt, np.ones(100))
    assert init.success and init.num_iterations == 0
    assert init.sim3_params.tobytes() == al.Sim3FromRotationTranslationScale(R, t, sc).tobytes()
    assert np.abs(init.sim3_params - ref.sim3_from_rts(*ref.umeyama(src, tgt))).max() < 1e-9
    # ... and a solve from there: noisy targets and per-point weights, so that the Umeyama result (unit weights) is near the
    # optimum but not at it and the final cost is far above rounding
    tgt_n = tgt + rng.normal(0.0, 0.01, size=tgt.shape)
    w = rng.uniform(0.5, 2.0, size=100)
    o = al.Sim3AlignmentOptions()
    o.start_from_initial_alignment = True
    o.set_point_weights(w)
    s3 = al.OptimizeAlignmentSim3(src, tgt_n, o)
    R, t, sc = al.AlignPointCloudsUmeyamaWithWeights(src, tgt_n, np.ones(100))
    b = ref.solve(ref.Problem(src, tgt_n, weights=w), al.Sim3FromRotationTranslationScale(R, t, sc), 100)
    assert b.successful >= 1 and b.final_cost > 1e-4
    assert s3.success == b.success and s3.num_iterations == b.num_iterations and s3.termination == b.termination
    assert np.abs(s3.sim3_params - b.params).max() < 1e-12
    # empty and mismatched inputs: the summary as constructed
    assert not al.OptimizeAlignmentSim3(np.zeros((0, 3)), np.zeros((0, 3))).success
    assert not al.OptimizeAlignmentSim3(src[:10], tgt[:5]).success
    assert al.OptimizeAlignmentSim3(src[:2], tgt[:2]).success                # "Should still work with small point clouds"
    o = al.Sim3AlignmentOptions()
    o.minimizer_type = "LINE_SEARCH"
    with pytest.raises(capi.TheiaHipError):
        al.OptimizeAlignmentSim3(src, tgt, o)
    # Sim3UtilityFunctionsTest (:438-463)
    Rx = ref.rotation_from_axis_angle([1.0, 0.0, 0.0], 0.5)
    tt, sc = np.array([1.0, 2.0, 3.0]), 1.5
    p = al.Sim3FromRotationTranslationScale(Rx, tt, sc)
    M = al.Sim3ToHomogeneousMatrix(p)
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = sc * Rx, tt
    assert np.abs(M - want).max() < 1e-12
    R2, t2, s2_ = al.Sim3ToRotationTranslationScale(p)
    assert np.linalg.norm(R2 - Rx) < 1e-12 and np.linalg.norm(t2 - tt) < 1e-12 and abs(s2_ - sc) < 1e-12
