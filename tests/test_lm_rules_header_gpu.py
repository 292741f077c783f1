"""GPU: the trust-region step rules of csrc/lm_rules.h, which every Levenberg-Marquardt loop of the library takes its rules
from.  theia_hip_selftest_lm_rules plays a script of step outcomes through the header in one device thread and on the host;
both must equal a plain restatement of Ceres' rules in float64 -- to the bit: everything is built from + - * / sqrt fmin fmax,
which IEEE 754 rounds in one way.  Only the radius of the pow form of the cube is compared at 1e-9 relative, the bound
compare_trace (tests/test_lm_rules_gpu.py) puts on the radius."""
import ctypes as C
import sys

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi

pytestmark = pytest.mark.gpu

INVALID, EVALUATED, BEFORE_STEP, PARAMETER, FUNCTION, DIAGONAL, JACOBI, MODEL3, MODEL6 = range(1, 10)
DBL_MAX = sys.float_info.max
BIG = 1e300   # a max_radius that never binds


def play(records):
    """(device, host) [n][7]: radius | decrease factor | invalid steps | successful | decision | value | floor reached."""
    rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 4)
    dev, host = np.full((len(rec), 7), np.nan), np.full((len(rec), 7), np.nan)
    capi.check(capi.lib().theia_hip_selftest_lm_rules(len(rec), capi.ptr(rec, C.c_double), capi.ptr(dev, C.c_double),
                                                      capi.ptr(host, C.c_double)))
    return dev, host


def model(n, a, b, c):
    H = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            H[i, j] = H[j, i] = a + (i * (i + 1) // 2 + j)
    g, y = b + np.arange(n), c - np.arange(n)
    return float(y @ g - 0.5 * (y @ H @ y))   # integer-valued inputs: exact in any order


def restate(records):
    """Ceres' rules, restated; column 5 of an evaluated step is the radius with the cube taken by pow."""
    radius, decrease, invalid, successful = np.float64(1e4), np.float64(2.0), 0, 1
    out = []
    with np.errstate(all="ignore"):
        for op, a, b, c in np.asarray(records, dtype=np.float64).reshape(-1, 4):
            decision, value = 0.0, 0.0
            if op == INVALID:
                invalid += 1
                decision = float(invalid < 5)
                if invalid < 5:
                    radius = radius / decrease; decrease = decrease * 2.0; successful = 0
            elif op == EVALUATED:
                invalid = 0
                decision = float(a > 1e-3)
                if a > 1e-3:
                    t = 2.0 * a - 1.0
                    value = np.fmin(b, radius / np.fmax(1.0 / 3.0, 1.0 - np.power(t, 3.0)))
                    radius = np.fmin(b, radius / np.fmax(1.0 / 3.0, 1.0 - t * t * t))
                    decrease = np.float64(2.0); successful = 1
                else:
                    radius = radius / decrease; decrease = decrease * 2.0; successful = 0
                    value = radius
            elif op == BEFORE_STEP:
                decision = float((successful and a <= b) or radius <= 1e-32)
            elif op == PARAMETER:
                decision = float(a <= c * (b + c))
            elif op == FUNCTION:
                decision = float(abs(a - b) <= c * a)
            elif op == DIAGONAL:
                value = np.fmin(np.fmax(a, 1e-6), 1e32) / b
            elif op == JACOBI:
                value = 1.0 / (1.0 + np.sqrt(a))
            elif op in (MODEL3, MODEL6):
                value = model(3 if op == MODEL3 else 6, a, b, c)
            out.append([radius, decrease, invalid, successful, decision, value, float(radius <= 1e-32)])
    return np.array(out, dtype=np.float64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check(records):
    """host == device == restatement, to the bit (the pow-form radius of evaluated steps: 1e-9 relative)."""
    assert len(records) <= 16
    dev, host = play(records)
    want = restate(records)
    ev = np.asarray(records, dtype=np.float64).reshape(-1, 4)[:, 0] == EVALUATED
    exact = np.ones(want.shape, bool)
    exact[ev, 5] = False
    for got, name in ((dev, "device"), (host, "host")):
        assert same_bits(got[exact], want[exact]), (name, got, want)
        assert np.all(np.abs(got[ev, 5] - want[ev, 5]) <= 1e-9 * np.abs(want[ev, 5])), (name, got[ev, 5], want[ev, 5])
        # the pow form against the multiply form
        assert np.all(np.abs(got[ev, 5] - got[ev, 0]) <= 1e-9 * np.abs(got[ev, 0])), (name, got[ev, 5], got[ev, 0])
    assert same_bits(dev[exact], host[exact])
    return dev


def rec(op, a=0.0, b=0.0, c=0.0):
    return [float(op), a, b, c]


def test_five_invalid_steps_fail_at_the_fifth():
    d = check([rec(INVALID)] * 5)
    assert list(d[:, 4]) == [1, 1, 1, 1, 0]
    assert list(d[:4, 0]) == [1e4 / 2, 1e4 / 8, 1e4 / 64, 1e4 / 1024]
    assert list(d[:, 2]) == [1, 2, 3, 4, 5] and d[4, 0] == d[3, 0] and d[4, 1] == d[3, 1]   # the failed state stays


def test_an_evaluated_step_ends_the_run_of_invalid_ones():
    d = check([rec(INVALID)] * 4 + [rec(EVALUATED, 0.0, BIG)] + [rec(INVALID)] * 4)
    assert np.all(d[[0, 1, 2, 3, 5, 6, 7, 8], 4] == 1) and list(d[:, 2]) == [1, 2, 3, 4, 0, 1, 2, 3, 4]


def test_the_divisor_doubles_per_rejection_and_starts_over_after_an_accepted_step():
    d = check([rec(EVALUATED, 0.0, BIG), rec(EVALUATED, -1.0, BIG), rec(EVALUATED, 0.5, BIG), rec(EVALUATED, 0.0, BIG)])
    assert list(d[:, 4]) == [0, 0, 1, 0] and list(d[:, 3]) == [0, 0, 1, 0]
    assert list(d[:, 0]) == [1e4 / 2, 1e4 / 8, 1e4 / 8, 1e4 / 16] and list(d[:, 1]) == [4, 8, 2, 4]


def test_rho_at_the_acceptance_threshold():
    d = check([rec(EVALUATED, 1e-3, BIG), rec(EVALUATED, np.nextafter(1e-3, 1.0), BIG), rec(EVALUATED, np.nan, BIG)])
    assert list(d[:, 4]) == [0, 1, 0]


def test_accepted_steps_scale_the_radius():
    d = check([rec(EVALUATED, 0.25, BIG), rec(EVALUATED, 0.5, BIG), rec(EVALUATED, 1.0, BIG), rec(EVALUATED, 2.0, BIG)])
    r0 = 1e4 / 1.125
    assert d[0, 0] == r0 and d[1, 0] == r0 and d[2, 0] == r0 / (1.0 / 3.0) and d[3, 0] == r0 / (1.0 / 3.0) / (1.0 / 3.0)
    assert np.all(d[:, 1] == 2.0) and np.all(d[:, 3] == 1)


def test_max_radius_clamps():
    d = check([rec(EVALUATED, 1.0, 2e4), rec(EVALUATED, 1.0, 2e4)])
    assert list(d[:, 0]) == [2e4, 2e4]


def test_fifteen_rejections_reach_the_radius_floor():
    d = check([rec(EVALUATED, 0.0, BIG)] * 15 + [rec(BEFORE_STEP, DBL_MAX, 0.0)])
    assert list(d[:, 6]) == [0] * 14 + [1, 1] and d[13, 0] > 1e-32 >= d[14, 0] and d[15, 4] == 1


def test_gradient_rule_after_successful_steps_only():
    tol = 1e-10
    d = check([rec(BEFORE_STEP, tol, tol),                                   # the start counts as successful
               rec(EVALUATED, 0.0, BIG), rec(BEFORE_STEP, 0.0, tol),         # rejected: ignored
               rec(INVALID), rec(BEFORE_STEP, 0.0, tol),
               rec(EVALUATED, 1.0, BIG), rec(BEFORE_STEP, tol, tol), rec(BEFORE_STEP, np.nextafter(tol, 1.0), tol),
               rec(BEFORE_STEP, np.nan, tol)])
    assert list(d[[0, 2, 4, 6, 7, 8], 4]) == [1, 0, 0, 1, 0, 0]


def test_parameter_and_function_rules_at_equality():
    tol, xn = 1e-8, 3.0
    edge = tol * (xn + tol)
    d = check([rec(PARAMETER, edge, xn, tol), rec(PARAMETER, np.nextafter(edge, 1.0), xn, tol), rec(PARAMETER, 0.0, 0.0, 0.0),
               rec(PARAMETER, np.inf, xn, tol), rec(PARAMETER, np.nan, xn, tol),
               rec(FUNCTION, 8.0, 8.0 - 8.0 * 2.0 ** -20, 2.0 ** -20), rec(FUNCTION, 8.0, 8.0 - 8.0 * 2.0 ** -19, 2.0 ** -20),
               rec(FUNCTION, 8.0, 8.0 + 8.0 * 2.0 ** -20, 2.0 ** -20), rec(FUNCTION, 0.0, 0.0, 0.0),
               rec(FUNCTION, 1.0, DBL_MAX, 1e-6), rec(FUNCTION, DBL_MAX, DBL_MAX, 0.0)])
    assert list(d[:, 4]) == [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1]


def test_lm_diagonal_and_jacobi_scale():
    d = check([rec(DIAGONAL, 0.0, 1e4), rec(DIAGONAL, 1e40, 1e4), rec(DIAGONAL, np.nan, 1e4), rec(DIAGONAL, 2.5, 3.0),
               rec(DIAGONAL, -1.0, 0.125), rec(JACOBI, 0.0), rec(JACOBI, 9.0), rec(JACOBI, 2.0), rec(JACOBI, 1e300)])
    assert list(d[:5, 5]) == [1e-6 / 1e4, 1e32 / 1e4, 1e-6 / 1e4, 2.5 / 3.0, 1e-6 / 0.125]
    assert list(d[5:7, 5]) == [1.0, 0.25]


def test_model_cost_change_on_a_packed_triangle():
    d = check([rec(MODEL3, 1.0, 2.0, 3.0), rec(MODEL6, 1.0, 2.0, 3.0), rec(MODEL3, -4.0, 0.0, 1.0), rec(MODEL6, 2.0, -7.0, 5.0)])
    # 3 x 3 by hand: H = [[1, 2, 4], [2, 3, 5], [4, 5, 6]], g = (2, 3, 4), y = (3, 2, 1): y'g = 16, Hy = (11, 17, 28), y'Hy = 95
    assert d[0, 5] == 16.0 - 47.5


def test_selftest_refuses_bad_arguments():
    L, E = capi.lib(), capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    v, o = np.zeros(4 * 17), np.zeros(7 * 17)
    p = lambda a: capi.ptr(a, C.c_double)     # noqa: E731
    assert L.theia_hip_selftest_lm_rules(0, p(v), p(o), p(o)) == E
    assert L.theia_hip_selftest_lm_rules(17, p(v), p(o), p(o)) == E
    assert L.theia_hip_selftest_lm_rules(1, None, p(o), p(o)) == E
    assert L.theia_hip_selftest_lm_rules(1, p(v), None, p(o)) == E
    assert L.theia_hip_selftest_lm_rules(1, p(v), p(o), None) == E
