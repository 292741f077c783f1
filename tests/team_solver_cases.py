"""Inputs and a 40-digit yardstick for the team eigen, SVD and five-point solvers (eig_team.h, svd_team.h, fit5_team.h) and
their one-thread and oracle copies (EISPACK orthes + hqr2, two-sided Jacobi SVD, five_point_pre).

Every family is deterministic (seeded by its name and n).  The yardstick is mpmath at 40 digits: mp.eig with left and right
vectors gives the eigenvalues and their condition numbers, mp.svd_r the singular values.  numpy is no yardstick here: LAPACK
balances and EISPACK does not, so the two differ far beyond u on graded matrices although both are right.  References are
cached for the session (at most about forty of the expensive ones)."""
import functools
import math
import zlib
from fractions import Fraction

import ctypes as C
import mpmath as mp
import numpy as np
from scipy.optimize import linear_sum_assignment

from pytheiasfm_amd import _capi as capi
from tests import oracle_lib as ol

U = 2.0 ** -53
DPS = 40

EIG_FAMILIES = ["gauss", "zero", "identity", "three_i", "diag_repeated", "diag_unsorted", "upper_tri", "hess_split",
                "rot_blocks", "cyclic", "reversal", "jordan", "nilpotent", "companion_clustered", "companion_complex",
                "rank1", "skew", "scaled_1e150", "scaled_1e-150", "graded", "nan", "inf"]
DEFECTIVE = {"jordan", "nilpotent", "companion_clustered"}   # eigenvalue bound on the trace instead (kappa is unbounded)
NONFINITE = {"nan", "inf"}
# n of each eigen variant: 0 = eig_team<8, false> (five-point, P4Pf: 10), 1 = eig_team<8, true> (UPnP 8, P4Pfr 13),
# 2 = eig_team<32, true, 4> (DLS, gDLS: 27; the kept rows {0, 9, 3, 1} need n >= 10)
VARIANT_N = {0: [1, 2, 3, 5, 10], 1: [1, 2, 3, 8, 10, 13], 2: [10, 16, 27]}
VARIANT_CPLX = {0: False, 1: True, 2: True}
KEPT_ROWS = [0, 9, 3, 1]
REF_N = (1, 2, 3, 10)   # every family has an mpmath reference at these n (10: an n of all three variants)

SVD_FAMILIES = ["gauss", "rank0", "rank1", "rank8", "repeated", "negative_diag", "permutation", "scaled_1e150",
                "scaled_1e-150", "graded", "omega"]
FP_FAMILIES = ["random", "small_int", "half_int", "duplicated", "collinear"]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _companion(roots):
    c = np.real(np.poly(roots))
    n = len(roots)
    A = np.zeros((n, n))
    A[0, :] = -c[1:] / c[0]
    A[np.arange(1, n), np.arange(n - 1)] = 1.0
    return A


def eig_matrix(family, n):
    """The n x n member of an eigen family (float64, row-major)."""
    rng = _rng("eig", family, n)
    G = rng.normal(size=(n, n))
    I = np.eye(n)
    if family == "gauss":
        return G
    if family == "zero":
        return np.zeros((n, n))
    if family == "identity":
        return I
    if family == "three_i":
        return 3.0 * I
    if family == "diag_repeated":
        return np.diag(np.array([2.0, -1.0, 2.0, 0.5, -1.0])[np.arange(n) % 5])
    if family == "diag_unsorted":
        return np.diag(((np.arange(n) * 7) % n + 1.0) * (-1.0) ** np.arange(n))
    if family == "upper_tri":
        return np.triu(G)
    if family == "hess_split":   # Hessenberg with one exactly-zero subdiagonal entry
        H = np.triu(G, -1)
        if n >= 2:
            H[n // 2, n // 2 - 1] = 0.0
        return H
    if family == "rot_blocks":   # only complex pairs (a real 0.5 when n is odd)
        A = np.zeros((n, n))
        for k in range(n // 2):
            t = 0.3 + 0.7 * k
            A[2 * k:2 * k + 2, 2 * k:2 * k + 2] = [[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]
        if n % 2:
            A[n - 1, n - 1] = 0.5
        return A
    if family == "cyclic":
        return np.roll(I, 1, axis=0)
    if family == "reversal":
        return I[::-1].copy()
    if family == "jordan":
        return 2.0 * I + np.eye(n, k=1)
    if family == "nilpotent":
        return np.eye(n, k=1)
    if family == "companion_clustered":
        return _companion(1.0 + 1e-3 * (np.arange(n) - n / 2) / max(n, 1))
    if family == "companion_complex":
        roots = [0.9 * np.exp(1j * (0.4 + 2.5 * k / n)) for k in range(n // 2)]
        roots = roots + [np.conj(r) for r in roots] + ([0.3] if n % 2 else [])
        return _companion(np.array(roots))
    if family == "rank1":
        return np.outer(rng.normal(size=n), rng.normal(size=n))
    if family == "skew":
        return G - G.T
    if family == "scaled_1e150":
        return G * 1e150
    if family == "scaled_1e-150":
        return G * 1e-150
    if family == "graded":   # 10^k rows and columns
        d = 10.0 ** np.linspace(0.0, 4.0, n)
        return d[:, None] * G * d[None, :]
    if family == "nan":
        G[n // 2, n // 3] = np.nan
        return G
    if family == "inf":
        G[n // 3, n // 2] = np.inf
        return G
    raise KeyError(family)


# ---- action matrices of the production solvers, from the oracle's exports on the existing scene generators
def _dls_actions(count, seed):
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dls_reference_vectors.json")))
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    while len(out) < count:
        if k < len(g["cases"]):
            D = np.array(g["cases"][k]["D"], dtype=np.float64); u = np.array(g["cases"][k]["u"], dtype=np.float64)
        else:
            M = rng.normal(size=(9, 9)); D = (M @ M.T).ravel(); u = rng.uniform(-100.0, 100.0, 4)
        k += 1
        fc = np.zeros(375); A = np.zeros((27, 27))
        if ol.rlib().oracle_dls_action_from_cost(capi.ptr(D, C.c_double), capi.ptr(u, C.c_double), capi.ptr(fc, C.c_double),
                                                 capi.ptr(A, C.c_double)):
            out.append(A)
    return out


def _upnp_actions(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        s = np.array([q[0] ** 2, q[1] ** 2, q[2] ** 2, q[3] ** 2, q[0] * q[1], q[0] * q[2], q[0] * q[3], q[1] * q[2], q[1] * q[3],
                      q[2] * q[3]])
        Mh = rng.normal(size=(10, 10)); A = Mh @ Mh.T; A = 0.5 * (A + A.T)
        out.append(ol.upnp_action_matrix(A, -A @ s))
    return out


def _p4pf_actions(count, seed):
    from tests import p4pf_scenes as ps
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        _, X, px, _ = ps.random_scene(rng)
        T = np.zeros((10, 10))
        if ol.rlib().oracle_p4pf_action(capi.ptr(np.ascontiguousarray(np.concatenate([px, X], axis=1)), C.c_double),
                                        capi.ptr(T, C.c_double)) == 1:
            out.append(T)
    return out


def _p4pfr_actions(count, seed):
    from tests import p4pfr_scenes as sc
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        f, W, _, _ = sc.solver_scene("basic", noise=0.5, rng=rng)
        _, _, A = ol.p4pfr_solve(f, W, rng.uniform(-0.5, 0.5, 3), sc.SOLVER_LIMITS, want_matrices=True)
        if np.abs(A).max() > 0:
            out.append(A)
    return out


def _five_point_actions(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        ok, _, M = five_point_pre_oracle(rng.normal(size=(5, 4)) * 0.5)
        if ok:
            out.append(M)
    return out


ACTION_N = {"five_point": 10, "p4pf": 10, "upnp": 8, "p4pfr": 13, "dls": 27}
_ACTION_GEN = {"five_point": _five_point_actions, "p4pf": _p4pf_actions, "upnp": _upnp_actions, "p4pfr": _p4pfr_actions,
               "dls": _dls_actions}
VARIANT_ACTIONS = {0: ["five_point", "p4pf"], 1: ["upnp", "p4pfr"], 2: ["dls"]}


@functools.lru_cache(maxsize=None)
def _actions_cached(kind, count, seed):
    return tuple(_ACTION_GEN[kind](count, seed))


def action_matrices(kind, count, seed=1):
    return [a.copy() for a in _actions_cached(kind, count, seed)]


# ---- the oracle copies
def eig_oracle(A, cplx):
    """(ok, wr, wi, H, V): the oracle's eig_general_t (<10, false> or <27, true>).  H = the Schur form of a second run without
    vectors (the run with vectors back-substitutes into H)."""
    n = A.shape[0]
    ok, wr, wi, V = ol.eig_complex(A) if cplx else ol.eig(A)
    H = np.ascontiguousarray(A, dtype=np.float64).copy(); wr2 = np.zeros(n); wi2 = np.zeros(n)
    f = ol.rlib().oracle_eig_complex if cplx else ol.rlib().oracle_eig
    f.argtypes = [C.c_int, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p]
    ok2 = f(n, capi.ptr(H, C.c_double), capi.ptr(wr2, C.c_double), capi.ptr(wi2, C.c_double), None)
    assert bool(ok) == bool(ok2)
    if ok:
        assert np.array_equal(wr.view(np.int64), wr2.view(np.int64)) and np.array_equal(wi.view(np.int64), wi2.view(np.int64))
    return bool(ok), wr, wi, H, V


def five_point_pre_oracle(corr):
    corr = np.ascontiguousarray(corr, dtype=np.float64).reshape(5, 4)
    N = np.zeros((9, 4)); M = np.zeros((10, 10))
    L = ol.rlib()
    L.oracle_five_point_pre.argtypes = [capi.c_double_p, capi.c_double_p, capi.c_double_p]
    ok = L.oracle_five_point_pre(capi.ptr(corr, C.c_double), capi.ptr(N, C.c_double), capi.ptr(M, C.c_double))
    return bool(ok), N, M


# ---- the yardstick
def _fro(A):
    return math.sqrt(math.fsum(float(x) ** 2 for x in np.asarray(A, dtype=np.float64).ravel()))


@functools.lru_cache(maxsize=None)
def _mp_eig(key):
    A = eig_matrix(*key) if key[0] != "action" else action_matrices(key[1], key[2] + 1)[key[2]]
    n = A.shape[0]
    with mp.workdps(DPS):
        E, EL, ER = mp.eig(mp.matrix(A.tolist()), left=True, right=True)
        lam = np.array([complex(e) for e in E])
        kappa = np.empty(n)
        for i in range(n):
            x = ER[:, i]; y = EL[i, :]
            yx = mp.fsum(y[k] * x[k] for k in range(n))
            nx = mp.sqrt(mp.fsum(abs(x[k]) ** 2 for k in range(n))); ny = mp.sqrt(mp.fsum(abs(y[k]) ** 2 for k in range(n)))
            kappa[i] = float(nx * ny / abs(yx)) if yx != 0 else math.inf
    return A, lam, kappa


def eig_reference(family, n):
    """(A, eigenvalues, condition numbers) at 40 digits; family may be ("action", kind, index)."""
    return _mp_eig((family, n) if isinstance(family, str) else family)


def _ratio(err, bound):
    return 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)


def eig_accuracy(A, wr, wi, V, cplx, ref, defective):
    """Largest error / bound over the eigenvalues and the eigenvectors (hqr2 column convention), u = 2^-53:
    |lambda - lambda*| <= 32 n u |A|_F kappa(lambda*) after a multiset matching (normal matrices: kappa = 1; defective
    families and repeated eigenvalues of non-normal matrices: |sum lambda - tr A| <= 16 n u |A|_F instead), and
    |A v - lambda v| <= 32 n u |A|_F |v| for every real eigenvalue (and complex pair with cplx)."""
    n = A.shape[0]
    nA = _fro(A)
    _, lam_ref, kappa = ref
    lam = wr + 1j * wi
    normal = np.array_equal(A @ A.T, A.T @ A)
    sep = np.array([min([abs(lam_ref[i] - lam_ref[j]) for j in range(n) if j != i] or [math.inf]) for i in range(n)])
    simple = bool(np.all(sep > 1e-6 * max(nA, 1e-300)))
    worst = 0.0
    if defective or not (normal or simple):
        tr = math.fsum(np.diag(A)); s = math.fsum(wr)
        worst = max(worst, _ratio(abs(s - tr), 16 * n * U * nA))
        assert abs(math.fsum(wi)) <= 16 * n * U * nA
    else:
        cost = np.abs(lam[:, None] - lam_ref[None, :])
        r, c = linear_sum_assignment(cost)
        k = np.ones(n) if normal else kappa
        for i, j in zip(r, c):
            worst = max(worst, _ratio(cost[i, j], 32 * n * U * nA * k[j]))
    Al = A.astype(np.longdouble)
    for j in range(n):
        if wi[j] == 0.0:
            v = V[:, j].astype(np.longdouble)
            res = Al @ v - np.longdouble(wr[j]) * v
            nv = _fro(V[:, j])
            assert nv > 0.0, f"eigenvector {j} is zero"
            worst = max(worst, _ratio(math.sqrt(float(np.sum(res * res))), 32 * n * U * nA * nv))
        elif cplx and wi[j] > 0.0:
            vr = V[:, j].astype(np.longdouble); vi = V[:, j + 1].astype(np.longdouble)
            a, b = np.longdouble(wr[j]), np.longdouble(wi[j])
            rr = Al @ vr - (a * vr - b * vi); ri = Al @ vi - (a * vi + b * vr)
            nv = math.hypot(_fro(V[:, j]), _fro(V[:, j + 1]))
            assert nv > 0.0, f"eigenvector pair {j} is zero"
            worst = max(worst, _ratio(math.sqrt(float(np.sum(rr * rr) + np.sum(ri * ri))), 32 * n * U * nA * nv))
    return worst


def svd_matrix(family):
    rng = _rng("svd", family)
    G = rng.normal(size=(9, 9))
    Q1, _ = np.linalg.qr(rng.normal(size=(9, 9))); Q2, _ = np.linalg.qr(rng.normal(size=(9, 9)))
    if family == "gauss":
        return G
    if family == "rank0":
        return np.zeros((9, 9))
    if family == "rank1":
        return np.outer(rng.normal(size=9), rng.normal(size=9))
    if family == "rank8":
        return (Q1 * np.array([5, 4, 3, 2.5, 2, 1.5, 1, 0.5, 0.0])) @ Q2.T
    if family == "repeated":
        return (Q1 * np.array([3, 3, 3, 2, 2, 1, 1, 1, 0.5])) @ Q2.T
    if family == "negative_diag":
        return np.diag(-np.arange(1.0, 10.0)[::-1] * (1 + 0.1 * (np.arange(9) % 3)))
    if family == "permutation":
        return np.eye(9)[[3, 7, 0, 8, 1, 5, 2, 6, 4]]
    if family == "scaled_1e150":
        return G * 1e150
    if family == "scaled_1e-150":
        return G * 1e-150
    if family == "graded":
        d = 10.0 ** np.arange(0.0, 9.0) / 1e4
        return d[:, None] * G * d[None, :]
    if family == "omega":   # SQPnP's Omega: a rank-6 positive semidefinite 9 x 9 matrix
        B = rng.normal(size=(9, 6))
        return B @ B.T
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def svd_reference(family):
    A = svd_matrix(family)
    with mp.workdps(DPS):
        s = mp.svd_r(mp.matrix(A.tolist()), compute_uv=False)
        return np.array(sorted((float(x) for x in s), reverse=True))


def svd_accuracy(A, Uo, S, Vo, sref):
    """Largest error / bound: |sigma_i - sigma_i*| <= 16 * 9 u sigma_1*; U (V) orthonormal to 64 * 9 u; |A - U S V^T|_F <=
    64 * 9 u |A|_F.  S sorted descending and non-negative."""
    assert np.all(S >= 0.0) and np.all(np.diff(S) <= 0.0), S
    worst = max([_ratio(abs(S[i] - sref[i]), 16 * 9 * U * sref[0]) for i in range(9)])
    I = np.eye(9, dtype=np.longdouble)
    for Q in (Uo, Vo):
        if Q is not None:
            Ql = Q.astype(np.longdouble)
            worst = max(worst, _ratio(float(np.abs(Ql.T @ Ql - I).max()), 64 * 9 * U))
    if Vo is not None:
        R = A.astype(np.longdouble) - (Uo.astype(np.longdouble) * S.astype(np.longdouble)) @ Vo.astype(np.longdouble).T
        worst = max(worst, _ratio(math.sqrt(float(np.sum(R * R))), 64 * 9 * U * _fro(A)))
    return worst


def fp_corr(family, seed=0):
    """Five correspondences (5, 4) = (x1, y1, x2, y2)."""
    rng = _rng("fp", family, seed)
    if family == "random":
        return rng.normal(size=(5, 4)) * 0.5
    if family == "small_int":   # exact pivot ties in |a|
        return rng.integers(-3, 4, size=(5, 4)).astype(np.float64)
    if family == "half_int":
        return rng.integers(-6, 7, size=(5, 4)).astype(np.float64) / 2.0
    if family == "duplicated":
        c = rng.normal(size=(5, 4)) * 0.5
        c[4] = c[1]
        return c
    if family == "collinear":   # both images on a line: the system has rank 3
        t = np.arange(5.0) - 2.0
        return np.stack([t, 2 * t + 1, 0.5 * t - 1, -t + 3], axis=1)
    raise KeyError(family)


def fp_system(corr):
    """The 5 x 9 epipolar system exactly as the solvers form it (products rounded in double)."""
    x1, y1, x2, y2 = (corr[:, k] for k in range(4))
    return np.stack([x2 * x1, y2 * x1, x1, x2 * y1, y2 * y1, y1, x2, y2, np.ones(5)], axis=1)


def exact_rank(Q):
    M = [[Fraction(float(v)) for v in row] for row in Q]
    rank, rows, cols = 0, len(M), len(M[0])
    for c in range(cols):
        p = next((r for r in range(rank, rows) if M[r][c] != 0), None)
        if p is None:
            continue
        M[rank], M[p] = M[p], M[rank]
        for r in range(rows):
            if r != rank and M[r][c] != 0:
                f = M[r][c] / M[rank][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[rank])]
        rank += 1
    return rank


def fp_null_ratio(corr, N):
    """|Q N|_F / (64 * 9 u |Q|_F |N|_F): the null space is one at the level of u |Q|."""
    Q = fp_system(corr)
    R = Q.astype(np.longdouble) @ N.astype(np.longdouble)
    return _ratio(math.sqrt(float(np.sum(R * R))), 64 * 9 * U * _fro(Q) * _fro(N))
