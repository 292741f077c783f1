"""CPU tests of the Sim(3) alignment's host-and-device header and of its comparator (no GPU).

pytheiasfm_amd/csrc/sim3_device.h is compiled with the host compiler into tests/sim3_maps_check.cpp (the same text the
device compiles, without FMA contraction) and checked against tests/golden/sim3_maps.npz (mpmath, tests/golden/
make_sim3_maps_golden.py); tests/sim3_ref.py -- numpy maps, torch.func.jacfwd Jacobians, Ceres' loop restated -- is checked
against the same values and against the known answers of the reference's scenes (align_point_clouds_test.cc:269-574).

TOLERANCE OF THE MAPS.  Sophus' closed forms cancel badly near their thresholds (exp at sigma = 1e-9 is good to 1e-7 only),
so the unit is the error of the algorithm itself: the numpy restatement's largest error against the golden per calcW branch
(small sigma, small theta), relative to max(1, largest entry of the value).  The compiled header runs the same operations and
may differ in libm's and the operation order's last bits: it is allowed 4 x that (not less than 4 x 2^-52, one rounding of a
value of unit size).  Measured with numpy 2.x / glibc on x86-64:
    branch (small sigma, small theta)    exp          log
    (True,  True )                       5.0e-13      1.1e-16
    (False, True )                       8.2e-08      1.4e-16
    (True,  False)                       4.2e-10      6.4e-11
    (False, False)                       6.9e-08      1.6e-10
(the compiled header's own: the same to two digits in every row).

TOLERANCE OF THE DERIVATIVE.  The closed forms of calcW_derivatives divide sums that cancel by up to theta^4 or sigma^4, and
so does forward-mode differentiation of calcW: both carry an error of about eps / m^4, m = the smallest of theta and |sigma|
that is not in a small branch (where the coefficients are constants).  Points with m < 1e-3 compare rounding noise with
rounding noise and are left out; the others are held to 16 eps max(1, |J|) / m^4.  Against the true derivative (golden
exp_jac) the same bound holds except in the small-sigma branch's column d t / d sigma, where the Jets -- and sim3_exp_d,
which returns what they return -- differentiate the constant C = 1 and the truth is upsilon / 2: that column is asserted to
be what the Jets give, not the truth."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sim3_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = 2.0 ** -52
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "sim3_maps.npz"))
TANGENTS = GOLDEN["tangents"]
BRANCHES = [ref.branch(a) for a in TANGENTS]
AS_WRITTEN_START = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("sim3") / "sim3_maps_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pytheiasfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sim3_maps_check.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def run_check(exe, op, rows):
    text = "\n".join(op + " " + " ".join(repr(float(x)) for x in r) for r in rows) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    return np.array([[float(x) for x in line.split()] for line in r.stdout.strip().split("\n")])


def rel_err(value, golden):
    return float(np.abs(value - golden).max() / max(1.0, np.abs(golden).max()))


def numpy_exp(a):
    sR, t = ref.sim3_exp(a)
    return np.concatenate([sR.reshape(-1), t])


def numpy_log(v):
    return ref.sim3_log(v[0], v[1:10].reshape(3, 3), v[10:13])


def branch_errors(values, golden):
    """largest rel_err per calcW branch"""
    out = {}
    for b, v, g in zip(BRANCHES, values, golden):
        out[b] = max(out.get(b, 0.0), rel_err(v, g))
    return out


def map_tolerances():
    """(exp, log): per branch, 4 x the numpy restatement's own error against the golden"""
    e = branch_errors([numpy_exp(a) for a in TANGENTS], GOLDEN["exp_hi"])
    lg = branch_errors([numpy_log(v) for v in GOLDEN["log_in"]], GOLDEN["log_hi"])
    return ({b: 4.0 * max(v, EPS64) for b, v in e.items()}, {b: 4.0 * max(v, EPS64) for b, v in lg.items()}, e, lg)


def test_golden_covers_every_branch():
    assert set(BRANCHES) == {(True, True), (True, False), (False, True), (False, False)}
    assert len(TANGENTS) >= 60


def test_compiled_maps_against_golden(check_exe):
    tol_e, tol_l, err_e, err_l = map_tolerances()
    E = run_check(check_exe, "exp", TANGENTS)
    L = run_check(check_exe, "log", GOLDEN["log_in"])
    assert np.all(L[:, 0] == 1.0)
    got_e = branch_errors(E, GOLDEN["exp_hi"])
    got_l = branch_errors(L[:, 1:], GOLDEN["log_hi"])
    for b in sorted(got_e):
        print(f"branch {b}: exp numpy {err_e[b]:.2e} compiled {got_e[b]:.2e} | log numpy {err_l[b]:.2e} compiled {got_l[b]:.2e}")
    for b in got_e:
        assert got_e[b] <= tol_e[b], (b, got_e[b], tol_e[b])
        assert got_l[b] <= tol_l[b], (b, got_l[b], tol_l[b])


def test_compiled_conversions(check_exe):
    """from_rts is log with the reference's argument order; to_rts returns (R(omega), t, e^sigma) and matrix4 [sR t; 0 1]"""
    tol_e, tol_l, _, _ = map_tolerances()
    li = GOLDEN["log_in"]
    F = run_check(check_exe, "from", np.concatenate([li[:, 1:13], li[:, :1]], axis=1))
    Lg = run_check(check_exe, "log", li)
    assert np.array_equal(F, Lg)
    T = run_check(check_exe, "to", TANGENTS)
    M = run_check(check_exe, "mat", TANGENTS)
    E = run_check(check_exe, "exp", TANGENTS)
    for i, b in enumerate(BRANCHES):
        g = GOLDEN["exp_hi"][i]
        assert np.array_equal(M[i].reshape(4, 4)[:3, :3].reshape(-1), E[i][:9]) and np.array_equal(M[i].reshape(4, 4)[:3, 3], E[i][9:])
        assert np.array_equal(M[i][12:], [0.0, 0.0, 0.0, 1.0])
        assert rel_err(T[i][9:12], g[9:12]) <= tol_e[b]
        assert abs(T[i][12] - li[i][0]) <= 4.0 * EPS64 * li[i][0]               # scale = |q|^2 = e^sigma
        assert np.abs(T[i][:9] - li[i][1:10]).max() <= 16.0 * EPS64               # R(omega), entries of unit size


def test_round_trip_log_exp(check_exe):
    """log(exp(a)) = a for |omega| < pi, at the accuracy of the two maps' branches"""
    tol_e, tol_l, _, _ = map_tolerances()
    E = run_check(check_exe, "exp", TANGENTS)
    rows = []
    for a, e in zip(TANGENTS, E):
        sR = e[:9].reshape(3, 3)
        s = float(np.exp(a[6]))
        rows.append(np.concatenate([[s], (sR / s).reshape(-1), e[9:]]))
    L = run_check(check_exe, "log", rows)
    for i, (a, b) in enumerate(zip(TANGENTS, BRANCHES)):
        # exp's error moves log's argument, and log's own error adds; pi - 1e-6: the quaternion's w = 5e-7 divides R's rounding
        near_pi = np.linalg.norm(a[3:6]) > 3.14
        tol = (tol_e[b] + tol_l[b]) * (1e7 if near_pi else 8.0)
        assert rel_err(L[i][1:], a) <= tol, (i, a, L[i][1:], tol)


def jacobian_floor(a):
    """m of the module docstring, or None where the comparison is rounding noise against rounding noise"""
    ssig, srot = ref.branch(a)
    m = min(1.0, 1.0 if srot else float(np.linalg.norm(a[3:6])), 1.0 if ssig else abs(float(a[6])))
    return m if m >= 1e-3 else None


def test_compiled_exp_derivative(check_exe):
    D = run_check(check_exe, "expd", TANGENTS)
    E = run_check(check_exe, "exp", TANGENTS)
    checked = 0
    for i, a in enumerate(TANGENTS):
        assert np.array_equal(D[i][:12], E[i])                                    # the value does not depend on the derivative
        m = jacobian_floor(a)
        if m is None:
            continue
        checked += 1
        J = np.concatenate([D[i][12:75].reshape(9, 7), D[i][75:].reshape(3, 7)])
        Jf = ref.exp_jacobian(a)
        tol = 16.0 * EPS64 * max(1.0, np.abs(Jf).max()) / m ** 4
        assert np.abs(J - Jf).max() <= tol, (i, a, np.abs(J - Jf).max(), tol)
        Jt = GOLDEN["exp_jac"][i].copy()
        if BRANCHES[i][0]:
            assert np.array_equal(J[9:, 6], np.zeros(3))                          # the Jets' derivative of C = 1, A and B
            Jt[9:, 6] = 0.0
        assert np.abs(J - Jt).max() <= tol + 1e-11, (i, a, np.abs(J - Jt).max(), tol)
    assert checked >= 40


def _errors(params, gt):
    R, t, s = ref.sim3_to_rts(params)
    Rg, tg, sg = ref.sim3_to_rts(gt)
    return float(np.linalg.norm(R - Rg)), float(np.linalg.norm(t - tg)), abs(s - sg)


GT = dict(translation=[1.0, 2.0, 0.5], rotation=[0.1, 0.05, 0.02], scale=1.5)


def _scene(n=100, noise=0.01, seed=11, gt=GT):
    rng = np.random.default_rng(seed)
    src = ref.synthetic_cloud(n, noise, rng)
    g = ref.create_sim3(gt["translation"], gt["rotation"], gt["scale"])
    return src, ref.transform_cloud(src, g), g


def test_reference_scene_point_to_point():
    src, tgt, gt = _scene()
    r = ref.solve(ref.Problem(src, tgt, ref.POINT_TO_POINT), AS_WRITTEN_START, 100)
    re, te, se = _errors(r.params, gt)
    assert r.success and re < 0.1 and te < 0.1 and se < 0.1 and r.alignment_error < 0.1


def test_reference_scene_robust():
    src, tgt, gt = _scene()
    tgt = tgt.copy()
    tgt[:5] += [2.0, 2.0, 2.0]
    r = ref.solve(ref.Problem(src, tgt, ref.ROBUST_POINT_TO_POINT, huber_threshold=0.5), AS_WRITTEN_START, 100)
    assert r.success and r.alignment_error < 5.0


def test_reference_scene_point_to_plane():
    src, tgt, gt = _scene()
    normals = np.tile([0.0, 0.0, 1.0], (100, 1))
    r = ref.solve(ref.Problem(src, tgt, ref.POINT_TO_PLANE, normals=normals), AS_WRITTEN_START, 100)
    assert r.success
    # Constant normals see z only: x and y of the translation stay where the start leaves them.  From the as-written
    # start (translation 0) the comparator ends 3.44 from the true translation (rotation 0.15, scale 2e-12), which the
    # reference's lenient 1.0 cannot hold; from the Umeyama start, as the reference's comments intend, it does.
    assert _errors(r.params, gt)[1] > 1.0
    r2 = ref.solve(ref.Problem(src, tgt, ref.POINT_TO_PLANE, normals=normals), ref.sim3_from_rts(*ref.umeyama(src, tgt)), 100)
    re, te, se = _errors(r2.params, gt)
    assert r2.success and re < 1.0 and te < 1.0 and se < 1.0


def test_reference_scene_initial_guess():
    src, tgt, gt = _scene()
    guess = ref.create_sim3([0.5, 1.0, 0.2], [0.05, 0.02, 0.01], 1.2)
    for start in (AS_WRITTEN_START, guess):                                       # as written, and as the comments intend
        r = ref.solve(ref.Problem(src, tgt), start, 50)
        re, te, se = _errors(r.params, gt)
        assert r.success and re < 0.1 and te < 0.1 and se < 0.1


@pytest.mark.parametrize("gt", [dict(translation=[0.0, 0.0, 0.0], rotation=[0.0, 0.0, 0.0], scale=1.0),
                                dict(translation=[1.0, 0.0, 0.0], rotation=[0.1, 0.0, 0.0], scale=1.2),
                                dict(translation=[5.0, 3.0, 2.0], rotation=[0.5, 0.3, 0.2], scale=2.0)])
def test_reference_scene_convergence(gt):
    src, tgt, _ = _scene(50, 0.05, 12, gt)
    r = ref.solve(ref.Problem(src, tgt), AS_WRITTEN_START, 200)
    assert r.success and r.final_cost < 1e-3 and r.num_iterations < 200


def test_comparator_counts_as_ceres_does():
    """summary.iterations.size(): iteration 0 counts; max_iterations = 1 leaves two; a start at the optimum leaves one"""
    src, tgt, gt = _scene(noise=0.0)
    r = ref.solve(ref.Problem(src, tgt), AS_WRITTEN_START, 1)
    assert r.termination == ref.TERM_MAX_ITERATIONS and not r.success and r.num_iterations == 2
    r = ref.solve(ref.Problem(src, tgt), gt, 100)
    assert r.termination == ref.TERM_GRADIENT and r.success and r.num_iterations == 1
    r = ref.solve(ref.Problem(np.zeros((0, 3)), np.zeros((0, 3))), AS_WRITTEN_START, 100)
    assert r.termination == ref.TERM_NO_POINTS and not r.success


def test_sum_dtype_spread_is_rounding():
    """the float64 and longdouble runs of the comparator (the yardstick of the GPU tests) agree to rounding on a plain scene"""
    src, tgt, _ = _scene()
    a = ref.solve(ref.Problem(src, tgt), AS_WRITTEN_START, 100, np.float64)
    b = ref.solve(ref.Problem(src, tgt), AS_WRITTEN_START, 100, np.longdouble)
    assert a.num_iterations == b.num_iterations and a.termination == b.termination
    assert np.abs(a.params - b.params).max() < 1e-12
