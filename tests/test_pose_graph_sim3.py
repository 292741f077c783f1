"""CPU tests of the Sim(3) pose graph: the comparator tests/pose_graph_sim3_ref.py (the reference's term, Sim3Manifold::Plus,
Ceres' loop) on its own, the device's per-edge text pytheiasfm_amd/csrc/pose_graph_sim3_device.h compiled by the host
compiler (tests/pose_graph_sim3_check.cpp, without FMA contraction) against it, and the ctypes structs.  The scenes and the
term cases of tests/test_pose_graph_sim3_gpu.py live here, with the CPU check that their seed is stable.

THE JACOBIAN'S CONVENTION.  The reference's J_i = sqrt_information (I + Jr0 / 2 + Jr0^2 / 12) Adj(exp(x_j)) is the derivative
of the residual along Sim3Manifold::Plus (x_i -> log(exp(x_i) exp(d))), as a series truncated after the second order in the
residual; J_j = -J_i likewise.  Central differences along Plus (h = 1e-6) agree with it at residual norms <= 0.05 to 2.4e-8,
measured here with the full information matrix of the test (entries up to 2; the adjoint of poses 2 away from the origin
multiplies the series' truncation error, O(|r|^4 / 720) = 9e-9 at 0.05); the bound is 1e-7.
Differences in the ambient 7-vector do NOT agree (1.6 apart here): the term is paired with an identity PlusJacobian and
only makes sense along Plus.

BOUND OF THE TERM (used here for the host build and in the GPU file for the device): as tests/test_sim3_alignment.py does
for the maps, the unit is the error of the algorithm itself -- the numpy term's largest error against the same formulas in
mpmath (50 digits), relative to the record's largest entry, per class of case; 4 x that, floored at 2^-52, is allowed.
Sophus' logarithm cancels near pi and near its thresholds in numpy exactly as on the device."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pose_graph_sim3_ref as pg
from tests import sim3_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = 2.0 ** -52
SEED = 11
SCENE_SIZES = (2, 3, 8, 65, 200)           # nodes; the odd-numbered scenes carry a full sqrt_information
TERM_COUNTS = (1, 63, 64, 65, 257)


# ---- the scenes of the solves
@functools.lru_cache(maxsize=None)
def scene(n):
    return pg.ring_scene(n, SEED + n, with_information=(SCENE_SIZES.index(n) % 2 == 1))


def moved_scene(n):
    """the scene with every start node (but the held one), measurement and information entry moved by one unit in the last
    place, random signs"""
    g, _ = scene(n)
    rng = np.random.default_rng(SEED + 1000 + n)

    def move(a):
        return a * (1.0 + EPS64 * rng.choice([-1.0, 1.0], size=a.shape))
    x = g.x0.copy()
    x[1:] = move(x[1:])
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    return pg.Graph(x, g.edges, move(g.z), None if g.W is None else move(g.W), fixed)


@functools.lru_cache(maxsize=None)
def expected(n):
    """the comparator's runs, once per scene: float64 sums, longdouble sums, float64 sums on moved inputs"""
    g, _ = scene(n)
    return pg.solve(g, sum_dtype=np.float64), pg.solve(g, sum_dtype=np.longdouble), pg.solve(moved_scene(n))


def counts(r):
    return (r.termination, r.iterations, r.successful, r.unsuccessful, r.invalid)


# ---- the cases of the term
CLASSES = ("omega = 0", "sigma = 0", "both zero", "x_i = x_j, identity", "all zero", "quat branch x", "quat branch y",
           "quat branch z", "random")


@functools.lru_cache(maxsize=None)
def term_cases():
    """257 edges: x_i, x_j, z [257][7], W [257][7][7] (full), class index [257].  The first eight are the special cases, one
    each; the rest are random with rotations up to 2.5 rad, |sigma| up to 0.7, and every 16th again a special case."""
    rng = np.random.default_rng(SEED + 7)
    n = max(TERM_COUNTS)
    xi, xj, z = (rng.uniform(-1.0, 1.0, size=(n, 7)) * np.array([2, 2, 2, 1.4, 1.4, 1.4, 0.7]) for _ in range(3))
    W = np.tile(np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5]), (n, 1, 1)) + 0.3 * rng.standard_normal((n, 7, 7))
    cls = np.full(n, len(CLASSES) - 1)
    for e in range(n):
        k = e if e < 8 else (e // 16) % 8 if e % 16 == 0 else -1
        if k < 0:
            continue
        cls[e] = k
        if k in (0, 2):
            xi[e, 3:6] = xj[e, 3:6] = z[e, 3:6] = 0.0
        if k in (1, 2):
            xi[e, 6] = xj[e, 6] = z[e, 6] = 0.0
        if k == 3:
            xj[e] = xi[e]
            z[e] = 0.0
        if k == 4:
            xi[e] = xj[e] = z[e] = 0.0
        if k >= 5:        # the error's rotation is z's: 2.9 rad about one axis, trace < 0, largest diagonal entry k - 5
            xi[e] = xj[e] = 0.0
            z[e, 3:6] = 0.02 * rng.standard_normal(3)
            z[e, 3 + (k - 5)] = 2.9
    return xi, xj, z, W, cls


@functools.lru_cache(maxsize=None)
def term_expected(weighted):
    """per edge the comparator's record (residual [7] | J_i [49]), the mpmath record, and the allowed deviation: 4 x the
    class's largest relative comparator error (floored at 2^-52) x the record's largest entry"""
    xi, xj, z, W, cls = term_cases()
    got, hi = [], []
    for e in range(len(cls)):
        w = W[e] if weighted else None
        r, J = pg.term(xi[e], xj[e], z[e], w)
        rm, Jm = pg.term_mp(xi[e], xj[e], z[e], w)
        got.append(np.concatenate([r, J.reshape(-1)]))
        hi.append(np.concatenate([rm, Jm.reshape(-1)]))
    got, hi = np.array(got), np.array(hi)
    size = np.abs(hi).max(1)
    rel = np.abs(got - hi).max(1) / size
    unit = np.array([max(rel[cls == c].max(), EPS64) for c in range(len(CLASSES))])
    return got, hi, 4.0 * unit[cls] * size, {CLASSES[c]: float(rel[cls == c].max()) for c in range(len(CLASSES))}


def check_term_records(records, weighted, count, label):
    """`records` [count][56] of the device text against the comparator under the module's bound -> the largest deviation in
    units of the bound"""
    got, hi, allowed, _ = term_expected(weighted)
    dev = np.abs(records - got[:count]).max(1)
    worst = float((dev / allowed[:count]).max())
    print(f"{label}: E {count} weighted {weighted}: largest deviation {dev.max():.2e}, {worst:.2f} x the bound")
    assert np.all(dev <= allowed[:count]), (label, count, int(np.argmax(dev / allowed[:count])), worst)
    return worst


def _fd(f, h=1e-6):
    return np.stack([(f(h * e) - f(-h * e)) / (2.0 * h) for e in np.eye(7)], axis=1)


def test_jacobian_is_the_derivative_along_plus_not_the_ambient_one():
    rng = np.random.default_rng(SEED + 1)
    worst_plus, worst_ambient = 0.0, 0.0
    for _ in range(6):
        xi, xj = (rng.uniform(-1.0, 1.0, size=7) * np.array([2, 2, 2, 1.0, 1.0, 1.0, 0.5]) for _ in range(2))
        d = rng.standard_normal(7)
        r0 = 0.05 * d / np.linalg.norm(d) * rng.uniform(0.2, 0.99)         # the residual: Sji = exp(r0) exp(x_j) exp(x_i)^-1
        z = pg.log(pg.mul(pg.group(r0), pg.mul(pg.group(xj), pg.inv(pg.group(xi)))))
        W = np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5]) + 0.1 * rng.standard_normal((7, 7))
        r, J = pg.term(xi, xj, z, W)
        assert np.linalg.norm(np.linalg.solve(W, r)) <= 0.05
        Ji = _fd(lambda e: pg.term(pg.plus(xi, e), xj, z, W, jac=False)[0])
        Jj = _fd(lambda e: pg.term(xi, pg.plus(xj, e), z, W, jac=False)[0])
        Ja = _fd(lambda e: pg.term(xi + e, xj, z, W, jac=False)[0])
        worst_plus = max(worst_plus, np.abs(Ji - J).max(), np.abs(Jj + J).max())
        worst_ambient = max(worst_ambient, np.abs(Ja - J).max())
    print(f"along Plus {worst_plus:.2e} (bound 1e-7), ambient {worst_ambient:.2e}")
    assert worst_plus <= 1e-7
    assert worst_ambient >= 1e-2


def test_plus_clamps_the_scale_step_at_minus_20():
    x = np.array([0.3, -0.2, 0.5, 0.1, 0.4, -0.3, 0.2])
    d = np.array([0.01, 0.02, -0.01, 0.02, 0.0, 0.01, -35.0])
    at = d.copy()
    at[6] = -20.0
    assert np.array_equal(pg.plus(x, d), pg.plus(x, at))
    assert abs(pg.plus(x, at)[6] - (0.2 - 20.0)) < 1e-9
    above = d.copy()
    above[6] = -19.0
    assert abs(pg.plus(x, above)[6] - (0.2 - 19.0)) < 1e-9
    assert np.abs(pg.plus(x, np.zeros(7)) - x).max() < 1e-14


def test_noisy_ring_with_one_held_node_reaches_its_ground_truth():
    g, gt = pg.ring_scene(8, SEED, noise=0.0, drift=0.05)
    assert np.abs(g.x0 - gt).max() > 0.05
    r = pg.solve(g)
    assert r.termination in (pg.TERM_GRADIENT, pg.TERM_FUNCTION, pg.TERM_PARAMETER) and r.successful >= 2
    assert r.final_cost < 1e-12 * r.initial_cost
    assert np.abs(r.nodes - gt).max() < 1e-6
    assert np.array_equal(r.nodes[0], g.x0[0])


def test_seed_is_stable():
    """for SEED the comparator's float64 run, its longdouble run and its run on inputs moved by one unit in the last place
    agree on the termination and every count, on every scene of the GPU file: the comparator alone needs no excuse"""
    for n in SCENE_SIZES:
        a, b, c = expected(n)
        print(n, counts(a), f"cost {a.initial_cost:.3e} -> {a.final_cost:.3e}, last relative change {a.last_rel_change:.2e}")
        assert counts(a) == counts(b) == counts(c), n
        assert np.array_equal(a.trace[:, 4], b.trace[:, 4]) and np.array_equal(a.trace[:, 4], c.trace[:, 4])
        assert a.successful >= 1


def test_mpmath_term_agrees_with_the_numpy_term():
    """the two restatements are written apart: 1e-9 of the record's size (the worst class, rotations of 2.9 rad, measures
    4e-14) says they state the same formulas"""
    for weighted in (False, True):
        _, _, _, rel = term_expected(weighted)
        print(weighted, {k: f"{v:.1e}" for k, v in rel.items()})
        assert max(rel.values()) < 1e-9


def test_special_cases_of_the_term():
    xi, xj, z, W, cls = term_cases()
    assert [int(c) for c in cls[:8]] == list(range(8))
    e = 4                                                # everything zero: exact
    r, J = pg.term(xi[e], xj[e], z[e], W[e])
    assert np.array_equal(r, np.zeros(7)) and np.array_equal(J, W[e])
    e = 3                                                # x_i = x_j, identity measurement: r = 0, J_i = sqrt_information Adj
    r, J = pg.term(xi[e], xj[e], z[e], W[e])
    A = W[e] @ pg.adjoint(pg.group(xj[e]))
    assert np.abs(r).max() <= 64 * EPS64 and np.abs(J - A).max() <= 64 * EPS64 * np.abs(A).max()
    for k in range(3):                                   # the three largest-diagonal branches of Eigen's quaternion
        R = pg.mul(pg.group(z[5 + k]), pg.mul(pg.group(xi[5 + k]), pg.inv(pg.group(xj[5 + k]))))[1]
        assert np.trace(R) < 0.0 and int(np.argmax(np.diag(R))) == k


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("pg_sim3") / "pose_graph_sim3_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pytheiasfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pose_graph_sim3_check.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def run_check(exe, op, rows):
    text = "\n".join(op + " " + " ".join(repr(float(x)) for x in r) for r in rows) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-400:])
    return np.array([[float(x) for x in line.split()] for line in r.stdout.strip().split("\n")])


def test_device_text_on_the_host_against_the_comparator(check_exe):
    xi, xj, z, W, cls = term_cases()
    n = len(cls)
    out = run_check(check_exe, "term", np.concatenate([xi, xj, z, W.reshape(n, 49)], axis=1))
    assert np.all(out[:, 0] == 1.0)
    check_term_records(out[:, 1:], True, n, "host build")
    out = run_check(check_exe, "term1", np.concatenate([xi, xj, z], axis=1))
    assert np.all(out[:, 0] == 1.0)
    check_term_records(out[:, 1:], False, n, "host build")
    assert np.array_equal(out[4, 1:8], np.zeros(7)) and np.array_equal(out[4, 8:].reshape(7, 7), np.eye(7))
    # Plus: the clamp, and against the comparator on the random cases
    d = 0.1 * xj
    d[:8, 6] = [-35.0, -20.0, -19.0, -25.0, 0.0, -1e3, 3.0, -20.5]
    p = run_check(check_exe, "plus", np.concatenate([xi, d], axis=1))
    assert np.all(p[:, 0] == 1.0)
    want = np.array([pg.plus(a, b) for a, b in zip(xi, d)])
    assert np.abs(p[:, 1:] - want).max() <= 1e-12
    at = d[:1].copy()
    at[0, 6] = -20.0
    assert np.array_equal(run_check(check_exe, "plus", np.concatenate([xi[:1], at], axis=1))[0], p[0])
    # outside Sophus' scale range: refused, not aborted
    far = np.zeros((1, 14))
    far[0, 6], far[0, 13] = 20.0, 10.0
    assert run_check(check_exe, "plus", far)[0, 0] == 0.0 and pg.plus(far[0, :7], far[0, 7:]) is None


def test_struct_sizes():
    from pytheiasfm_amd import _capi as capi
    assert ctypes.sizeof(capi.PoseGraphSim3OptionsC) == 2 * 4 + 5 * 8
    assert ctypes.sizeof(capi.PoseGraphSim3SummaryC) == 8 * 4 + 6 * 8
    assert "theia_hip_pose_graph_sim3" in capi.EXPORTED_SYMBOLS
    assert "theia_hip_selftest_sim3_pose_graph_term" in capi.EXPORTED_SYMBOLS
