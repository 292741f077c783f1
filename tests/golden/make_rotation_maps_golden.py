"""Generates tests/golden/rotation_maps.npz: the cases of tests/test_wide_rotations_gpu.py's direct tests of the rotation
maps (theia_hip_selftest_rotation_maps, theia_hip_selftest_pairwise_rotation_error), their values in 50-digit arithmetic
(mpmath) and, per quantity, the largest error of the float64 restatements against those values -- the unit the device's
tolerance is stated in.

The 50-digit functions are the reference's piecewise definitions with Ceres' branch conditions, evaluated on the float64
inputs exactly: AngleAxisToRotationMatrix (theta^2 > eps: Rodrigues, else I + [w]x), RotationMatrixToQuaternion (trace >= 0,
else the largest diagonal entry), QuaternionToAngleAxis (sin^2 > 0 with the cos < 0 rule, else the factor 2), Eigen's
AngleAxis(Matrix3) scaled to a rotation vector, and PairwiseRotationError's residual log(R(w_j) R(w_i)' R(rel)') with
SoftLOneLoss' corrector.  The Jacobian is mpmath.diff of the residual with every branch held at the one the point takes.

Cases.  Angles 0, 1e-9, 1.4e-8 | 1.6e-8 (theta^2 = eps), 1e-3, 1, 2 | 2.1 (trace = 0), pi - 1e-3, pi - 1e-6, pi - 1e-9, pi;
each about the coordinate axes, the diagonal and three random axes.  Rotation maps: a = angle * axis, b a random
full-sphere vector.  Pairwise error: a residual rotation D of that angle and axis composed onto random full-sphere w_i and
rel (w_j = log(D R(rel) R(w_i)) rounded to float64), and two cases whose residual is zero to the bit.  Values are stored as
a float64 pair hi + lo.  branch_margin is the distance of the logarithm's branch decision from a tie (the diagonal axis ties
the three diagonal entries when the trace is negative: no branch is asserted there).
    python tests/golden/make_rotation_maps_golden.py"""
import os
import sys

import numpy as np
import torch
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import nonlinear_rotation_ref as nref          # noqa: E402
from tests import rotation_averaging_ref as rar           # noqa: E402
from tests.independent_lm import loss                     # noqa: E402

mp.dps = 50
EPS = mpf(2) ** -52
WIDTH = 0.1
PI64 = float(np.pi)
ANGLES = [0.0, 1e-9, 1.4e-8, 1.6e-8, 1e-3, 1.0, 2.0, 2.1, PI64 - 1e-3, PI64 - 1e-6, PI64 - 1e-9, PI64]
JACOBIAN_MAX_ANGLE = PI64 - 1e-3


def axes(rng):
    r = rng.standard_normal((3, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return np.concatenate([np.eye(3), np.full((1, 3), 1.0 / np.sqrt(3.0)), r])


def full_sphere(rng, k):
    v = rng.standard_normal((k, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return rng.uniform(0.0, PI64, size=k)[:, None] * v


# ---- 50 digits.  Matrices are lists of rows; `take` holds the branches of an earlier evaluation (None: decide here).
def m_rot(w, big=None):
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if big is None:
        big = t2 > EPS
    if not big:
        return [[mpf(1), -w[2], w[1]], [w[2], mpf(1), -w[0]], [-w[1], w[0], mpf(1)]], big
    th = mp.sqrt(t2)
    x, y, z = w[0] / th, w[1] / th, w[2] / th
    c, s = mp.cos(th), mp.sin(th)
    return [[c + x * x * (1 - c), x * y * (1 - c) - z * s, y * s + x * z * (1 - c)],
            [z * s + x * y * (1 - c), c + y * y * (1 - c), -x * s + y * z * (1 - c)],
            [-y * s + x * z * (1 - c), x * s + y * z * (1 - c), c + z * z * (1 - c)]], big


def m_mul(A, B, ta=False, tb=False):
    a = (lambda r, k: A[k][r]) if ta else (lambda r, k: A[r][k])
    b = (lambda k, c: B[c][k]) if tb else (lambda k, c: B[k][c])
    return [[sum(a(r, k) * b(k, c) for k in range(3)) for c in range(3)] for r in range(3)]


def m_log(E, take=None):
    """(angle-axis, (branch, has_sin, cos < 0), margin of the branch decision)"""
    d = [E[0][0], E[1][1], E[2][2]]
    trace = d[0] + d[1] + d[2]
    if take is None:
        if trace >= 0:
            branch, margin = 0, abs(trace)
        else:
            i = 0
            if d[1] > d[0]:
                i = 1
            if d[2] > d[i]:
                i = 2
            branch, margin = 1 + i, min([abs(trace)] + [d[i] - d[k] for k in range(3) if k != i])
    else:
        branch, margin = take[0], None
    q = [None] * 4
    if branch == 0:
        t = mp.sqrt(trace + 1)
        q[0] = t / 2
        t = 1 / (2 * t)
        q[1], q[2], q[3] = (E[2][1] - E[1][2]) * t, (E[0][2] - E[2][0]) * t, (E[1][0] - E[0][1]) * t
    else:
        i = branch - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(E[i][i] - E[j][j] - E[k][k] + 1)
        q[i + 1] = t / 2
        t = 1 / (2 * t)
        q[0] = (E[k][j] - E[j][k]) * t
        q[j + 1] = (E[j][i] + E[i][j]) * t
        q[k + 1] = (E[k][i] + E[i][k]) * t
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    has_sin = (s2 > 0) if take is None else take[1]
    if not has_sin:
        return [2 * q[1], 2 * q[2], 2 * q[3]], (branch, has_sin, False), margin
    st = mp.sqrt(s2)
    neg = (q[0] < 0) if take is None else take[2]
    two_theta = 2 * (mp.atan2(-st, -q[0]) if neg else mp.atan2(st, q[0]))
    k = two_theta / st
    return [q[1] * k, q[2] * k, q[3] * k], (branch, has_sin, neg), margin


def m_eigen_rotvec(R):
    t = R[0][0] + R[1][1] + R[2][2]
    q = [None] * 4   # x y z w
    if t > 0:
        t = mp.sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    n = mp.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    if n == 0:
        return [mpf(0)] * 3
    angle = 2 * mp.atan2(n, abs(q[3]))
    if q[3] < 0:
        n = -n
    return [angle * q[0] / n, angle * q[1] / n, angle * q[2] / n]


def m_angle_between(a, b):
    """The angle of exp(a) exp(b)', both taken as exact rotations (no small-angle branch)."""
    Ra, Rb = m_rot(a, True)[0] if any(a) else m_rot(a, False)[0], m_rot(b, True)[0] if any(b) else m_rot(b, False)[0]
    D = m_mul(Ra, Rb, tb=True)
    c = (D[0][0] + D[1][1] + D[2][2] - 1) / 2
    s = mp.sqrt((D[2][1] - D[1][2]) ** 2 + (D[0][2] - D[2][0]) ** 2 + (D[1][0] - D[0][1]) ** 2) / 2
    return mp.atan2(s, c)


def m_residual(wi, wj, wr, take=None):
    """(corrected residual, sqrt(rho'), branches, margin)"""
    Ri, bi = m_rot(wi, None if take is None else take[0])
    Rj, bj = m_rot(wj, None if take is None else take[1])
    Rr, br = m_rot(wr, None if take is None else take[2])
    E = m_mul(Rj, m_mul(Ri, Rr, ta=True, tb=True))
    r, lt, margin = m_log(E, None if take is None else take[3])
    s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    sr = (1 + s / (mpf(WIDTH) ** 2)) ** mpf(-0.25)
    return r, sr, (bi, bj, br, lt), margin


def vec(x):
    return [mpf(float(v)) for v in x]


def split(values):
    """mpf array -> (hi, lo) float64 arrays with hi + lo = the value to 32 digits"""
    flat = list(np.array(values, dtype=object).ravel())
    hi = np.array([float(v) for v in flat])
    lo = np.array([float(v - mpf(float(h))) for v, h in zip(flat, hi)])
    shape = np.array(values, dtype=object).shape
    return hi.reshape(shape), lo.reshape(shape)


if __name__ == "__main__":
    rng = np.random.default_rng(20240)
    ax = axes(rng)
    angle = np.repeat(ANGLES, len(ax))
    axis = np.tile(ax, (len(ANGLES), 1))
    n = len(angle)
    out = dict(width=WIDTH, jacobian_max_angle=JACOBIAN_MAX_ANGLE)

    # ---- the rotation maps
    a = angle[:, None] * axis
    b = full_sphere(rng, n)
    R, lg, ml, eg = [], [], [], []
    for k in range(n):
        Ra = m_rot(vec(a[k]))[0]
        R.append(Ra)
        lg.append(m_log(Ra)[0])
        ml.append(m_log(m_mul(Ra, m_rot(vec(b[k]))[0]))[0])
        eg.append(m_eigen_rotvec(Ra))
    R64 = rar.aa_to_R(a)
    log64, mul64 = rar.R_to_aa(R64), rar.multiply_rotations(a, b)
    err_R = max(abs(mpf(float(R64[k, r, c])) - R[k][r][c]) for k in range(n) for r in range(3) for c in range(3))
    err_log = max(m_angle_between(vec(log64[k]), lg[k]) for k in range(n))
    err_mul = max(m_angle_between(vec(mul64[k]), ml[k]) for k in range(n))
    for name, val in (("R", R), ("log", lg), ("mul", ml), ("eigen", eg)):
        out[f"maps_{name}_hi"], out[f"maps_{name}_lo"] = split(val)
    out.update(maps_a=a, maps_b=b, maps_angle=angle, err_R=float(err_R), err_log=float(err_log), err_mul=float(err_mul))
    print(f"rotation maps: {n} cases; float64 restatement against 50 digits: matrix {float(err_R / EPS):.2f} eps, "
          f"logarithm {float(err_log / EPS):.2f} eps, product {float(err_mul / EPS):.2f} eps (as rotations, rad)")

    # ---- the pairwise rotation error
    wi = np.concatenate([full_sphere(rng, n), np.zeros((2, 3))])
    wr = np.concatenate([full_sphere(rng, n), np.zeros((2, 3))])
    wj = np.zeros_like(wi)
    wi[n + 1] = wj[n + 1] = (1e-9, 0.0, 0.0)     # E = (I + [w]x)(I - [w]x) = I to the bit; case n: all three vectors zero
    for k in range(n):
        D = m_rot(vec(angle[k] * axis[k]))[0]
        Rj = m_mul(D, m_mul(m_rot(vec(wr[k]))[0], m_rot(vec(wi[k]))[0]))
        wj[k] = [float(v) for v in m_log(Rj)[0]]
    m = n + 2
    res, Ji, Jj, srs, branch, margin, has_jac = [], [], [], [], [], [], []
    for k in range(m):
        r, sr, take, mg = m_residual(vec(wi[k]), vec(wj[k]), vec(wr[k]))
        res.append(r); srs.append(sr); branch.append(take[3][0]); margin.append(float(mg))
        jac = k >= n or angle[k] <= JACOBIAN_MAX_ANGLE
        has_jac.append(jac)
        J = [[[mpf(0)] * 3 for _ in range(3)] for _ in range(2)]
        if jac:
            for side in range(2):
                for col in range(3):
                    for row in range(3):
                        def f(t, side=side, col=col, row=row):
                            x = [vec(wi[k]), vec(wj[k])]
                            x[side][col] += t
                            return m_residual(x[0], x[1], vec(wr[k]), take)[0][row]
                        J[side][row][col] = sr * mp.diff(f, 0)
        Ji.append(J[0]); Jj.append(J[1])
    has_jac = np.array(has_jac)
    # the float64 restatement: torch residual and reverse-mode Jacobian, the corrector from independent_lm.loss
    t = [torch.tensor(v) for v in (wi, wj, wr)]
    r64 = nref._res(*t).numpy()
    j64 = [x.numpy() for x in nref._jac(*t)]
    sr64 = np.sqrt(loss("softl1", WIDTH, (r64 * r64).sum(1))[1])
    err_res = max(m_angle_between(vec(r64[k]), res[k]) for k in range(m))
    err_sr = max(abs(mpf(float(sr64[k])) - srs[k]) for k in range(m))
    err_J = mpf(0)
    for k in np.nonzero(has_jac)[0]:
        for side, J in ((0, Ji), (1, Jj)):
            for row in range(3):
                for col in range(3):
                    err_J = max(err_J, abs(mpf(float(sr64[k] * j64[side][k, row, col])) - J[k][row][col]))
    for name, val in (("residual", res), ("sr", srs), ("Ji", Ji), ("Jj", Jj)):
        out[f"edge_{name}_hi"], out[f"edge_{name}_lo"] = split(val)
    out.update(edge_wi=wi, edge_wj=wj, edge_rel=wr, edge_angle=np.concatenate([angle, [0.0, 0.0]]),
               edge_branch=np.array(branch, dtype=np.int32), edge_branch_margin=np.array(margin), edge_has_jacobian=has_jac,
               err_residual=float(err_res), err_sr=float(err_sr), err_J=float(err_J))
    jmax = max(abs(v) for J in (Ji, Jj) for M in J for row in M for v in row)
    print(f"pairwise error: {m} cases, branches {np.bincount(branch, minlength=4)}, {int(has_jac.sum())} with a Jacobian "
          f"(largest entry {float(jmax):.3f}); float64 restatement against 50 digits: residual {float(err_res / EPS):.2f} eps "
          f"(as a rotation, rad), sqrt(rho') {float(err_sr / EPS):.2f} eps, Jacobian {float(err_J / EPS):.2f} eps")
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rotation_maps.npz"), **out)
