"""Generates tests/golden/sim3_maps.npz: the tangents of the Sim(3) map tests (tests/test_sim3_alignment.py,
tests/test_sim3_alignment_gpu.py) and the values of Sim3::exp and Sim3::log on them in multi-precision arithmetic (mpmath,
150 digits carried so that 50 are left after the cancellations at theta, sigma = 1e-12; stored as a float64 pair hi + lo).

exp is the TRUE map: sR = e^sigma R(omega) (Rodrigues), t = W upsilon with W = A Omega + B Omega^2 + C I and the closed forms
of sim_details.hpp:39-46, their limits taken where theta or sigma is exactly zero.  It is continuous across Sophus' 1e-10
branch thresholds, so one value serves both sides of them.  exp_jac is its derivative d(sR | t) / da [12][7] (central
differences, h = 1e-40).
log's input is what a caller holds, in float64: scale = fl(e^sigma), R = fl(R(omega)), t = fl(W upsilon).  Its value follows
the definition Sim3(RxSO3(scale, R), t).log() on exactly those numbers: Eigen's quaternion of R, scaled by sqrt(scale);
sigma = ln |q|^2; omega = 2 atan(|v| / w) / |v| v of the unit quaternion; upsilon = W(omega, sigma)^-1 t.

Tangents [upsilon, omega, sigma]: |omega| and |sigma| each in {0, 1e-12, 1e-9, 1e-3, 1} (all four branches of calcW, both
sides of its thresholds); |omega| in {pi - 1e-6, 3.1}; sigma = +-3; and random ones.  Axes and upsilon are random.
    python tests/golden/make_sim3_maps_golden.py"""
import os

import numpy as np
from mpmath import mp, mpf, matrix

mp.dps = 150
PI64 = float(np.pi)


def m_hat(o):
    return matrix([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])


def m_abc(theta, sigma):
    s = mp.exp(sigma)
    if sigma == 0:
        C = mpf(1)
        if theta == 0:
            return mpf(1) / 2, mpf(1) / 6, C
        return (1 - mp.cos(theta)) / theta ** 2, (theta - mp.sin(theta)) / theta ** 3, C
    C = (s - 1) / sigma
    if theta == 0:
        return ((sigma - 1) * s + 1) / sigma ** 2, (s * sigma ** 2 / 2 + s - 1 - sigma * s) / sigma ** 3, C
    a, b, c = s * mp.sin(theta), s * mp.cos(theta), theta ** 2 + sigma ** 2
    A = (a * sigma + (1 - b) * theta) / (theta * c)
    B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    return A, B, C


def m_w(omega, sigma):
    theta = mp.sqrt(omega[0] ** 2 + omega[1] ** 2 + omega[2] ** 2)
    A, B, C = m_abc(theta, sigma)
    Om = m_hat(omega)
    return A * Om + B * (Om * Om) + C * mp.eye(3)


def m_rot(omega):
    theta = mp.sqrt(omega[0] ** 2 + omega[1] ** 2 + omega[2] ** 2)
    if theta == 0:
        return mp.eye(3)
    K = m_hat([o / theta for o in omega])
    return mp.eye(3) + mp.sin(theta) * K + (1 - mp.cos(theta)) * (K * K)


def m_exp(a):
    a = [mpf(v) if isinstance(v, mpf) else mpf(float(v)) for v in a]
    ups, omega, sigma = matrix(a[:3]), a[3:6], a[6]
    sR = mp.exp(sigma) * m_rot(omega)
    t = m_w(omega, sigma) * ups
    return [sR[r, c] for r in range(3) for c in range(3)] + [t[r] for r in range(3)]


def m_log(scale, R, t):
    m = matrix(3, 3)
    for r in range(3):
        for c in range(3):
            m[r, c] = mpf(float(R[r, c]))
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    v = [mpf(0)] * 3
    if tr > 0:
        tt = mp.sqrt(tr + 1)
        w = tt / 2
        tt = mpf(1) / 2 / tt
        v = [(m[2, 1] - m[1, 2]) * tt, (m[0, 2] - m[2, 0]) * tt, (m[1, 0] - m[0, 1]) * tt]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tt = mp.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        v[i] = tt / 2
        tt = mpf(1) / 2 / tt
        w = (m[k, j] - m[j, k]) * tt
        v[j] = (m[j, i] + m[i, j]) * tt
        v[k] = (m[k, i] + m[i, k]) * tt
    ss = mp.sqrt(mpf(float(scale)))
    w, v = w * ss, [x * ss for x in v]
    sq = v[0] ** 2 + v[1] ** 2 + v[2] ** 2 + w ** 2
    sigma = mp.log(sq)
    nq = mp.sqrt(sq)
    w, v = w / nq, [x / nq for x in v]
    n = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    f = 2 / w if n == 0 else 2 * mp.atan(n / w) / n
    omega = [f * x for x in v]
    ups = mp.inverse(m_w(omega, sigma)) * matrix([mpf(float(x)) for x in t])
    return [ups[0], ups[1], ups[2]] + omega + [sigma]


def m_exp_jacobian(a, h=mpf(10) ** -40):
    """d(sR | t) / da [12][7] of the true map by central differences in 150 digits"""
    cols = []
    for k in range(7):
        up = [mpf(float(v)) for v in a]
        dn = list(up)
        up[k] += h
        dn[k] -= h
        eu, ed = m_exp(up), m_exp(dn)
        cols.append([float((x - y) / (2 * h)) for x, y in zip(eu, ed)])
    return np.array(cols).T


def pair(vals):
    hi = np.array([float(x) for x in vals])
    lo = np.array([float(x - mpf(h)) for x, h in zip(vals, hi)])
    return hi, lo


def tangents():
    rng = np.random.default_rng(20260412)

    def axis():
        a = rng.standard_normal(3)
        return a / np.linalg.norm(a)
    out = []
    small = [0.0, 1e-12, 1e-9, 1e-3, 1.0]
    sign = 1.0
    for th in small:
        for sg in small:
            out.append(np.concatenate([rng.uniform(-2, 2, 3), th * axis(), [sign * sg]]))
            sign = -sign
    for th in (PI64 - 1e-6, 3.1):
        for sg in (0.0, 1e-3, 1.0, -1.0):
            out.append(np.concatenate([rng.uniform(-2, 2, 3), th * axis(), [sg]]))
    for sg in (3.0, -3.0):
        for th in (0.0, 1e-3, 1.0, 3.1):
            out.append(np.concatenate([rng.uniform(-2, 2, 3), th * axis(), [sg]]))
    for _ in range(20):
        out.append(np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(0, 3.0) * axis(), [rng.uniform(-2, 2)]]))
    return np.array(out)


def main():
    A = tangents()
    exp_hi, exp_lo, exp_jac, log_in, log_hi, log_lo = [], [], [], [], [], []
    for a in A:
        e = m_exp(a)
        exp_jac.append(m_exp_jacobian(a))
        hi, lo = pair(e)
        exp_hi.append(hi); exp_lo.append(lo)
        R = m_rot([mpf(float(x)) for x in a[3:6]])
        R64 = np.array([[float(R[r, c]) for c in range(3)] for r in range(3)])
        scale64 = float(mp.exp(mpf(float(a[6]))))
        t64 = hi[9:12]
        log_in.append(np.concatenate([[scale64], R64.reshape(-1), t64]))
        hi, lo = pair(m_log(scale64, R64, t64))
        log_hi.append(hi); log_lo.append(lo)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim3_maps.npz")
    np.savez(path, tangents=A, exp_hi=np.array(exp_hi), exp_lo=np.array(exp_lo), exp_jac=np.array(exp_jac), log_in=np.array(log_in),
             log_hi=np.array(log_hi), log_lo=np.array(log_lo))
    print(f"wrote {path}: {len(A)} tangents")


if __name__ == "__main__":
    main()
