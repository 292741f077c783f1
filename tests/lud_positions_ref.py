"""numpy / scipy restatement of LeastUnsquaredDeviationPositionEstimator::EstimatePositions
(global_pose_estimation/least_unsquared_deviation_position_estimator.cc:75-213) with ConstrainedL1Solver
(math/constrained_l1_solver.cc:49-187), written from the reference's description, line by line:

  rows       per pair e = (i, j): c_j - c_i - s_e d_e, d_e = R_i' position_2 (GetRotatedTranslation, :63-70)
  bounds     one row s_e per pair against 1: A = [B; C], b = [0; 1]                            (:103-121, solver :49-91)
  x-update   x = (A'A)^-1 A'(b + z - u), A'A factored once                                   (:145)
  relax      ax_hat = alpha A x + (1 - alpha)(z + b)                                          (:146-148)
  z          ModifiedShrinkage(ax_hat - b + u, 1 / rho): soft threshold on the L1 rows, max(0, .) on the bounds
  u          u += ax_hat - z - b
  stop       r_norm < primal_eps && s_norm < dual_eps                                         (:150-168)

form="full" builds the (3E + E) x (3m + E) sparse A and solves A'A with a sparse direct factorisation; form="schur"
eliminates the scales (S = sum_e K_e (x) (I - d_e d_e' / D_e), D_e = |d_e|^2 + 1) and solves S with a dense Cholesky --
what the device does.  check_schur=True (full form) repeats every x-update through the Schur form and records the
largest relative difference.  Every convergence decision records its margin: how far (relative) the deciding
comparisons sit from their thresholds."""
import math
import time

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.rotation_averaging_ref import aa_to_R


class SolverOptions:   # ConstrainedL1Solver::Options, math/constrained_l1_solver.h:64-74
    def __init__(self, **kw):
        self.max_num_iterations = 1000
        self.rho = 10.0
        self.alpha = 1.2
        self.absolute_tolerance = 1e-4
        self.relative_tolerance = 1e-2
        for k, v in kw.items():
            setattr(self, k, v)


def _margin(value, threshold):
    return abs(value - threshold) / max(abs(threshold), 1e-300)


def rotated_translations(orientations, edges, rel):
    """GetRotatedTranslation: d_e = R_i' t_e (R_i from ceres' angle-axis conversion)."""
    R = aa_to_R(np.asarray(orientations, dtype=np.float64)[edges[:, 0]])
    return np.einsum("eji,ej->ei", R, np.asarray(rel, dtype=np.float64).reshape(-1, 3))


def lud_positions(orientations, edges, rel, fixed=None, options=None, form="full", check_schur=False):
    """Returns a dict: positions [n][3] (held views at the origin), scales [E], admm_iterations, converged, margins
    (one per iteration), final_margins (the last two), r_norm, s_norm, primal_eps, dual_eps, schur_max_rel
    (check_schur), cpu_ms."""
    t0 = time.perf_counter()
    o = options or SolverOptions()
    orientations = np.asarray(orientations, dtype=np.float64).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n, E = orientations.shape[0], edges.shape[0]
    fix = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool).copy()
    if not fix.any():
        fix[0] = True
    idx = -np.ones(n, dtype=np.int64)
    free = np.nonzero(~fix)[0]
    m = len(free)
    idx[free] = np.arange(m)
    ei, ej = idx[edges[:, 0]], idx[edges[:, 1]]
    d = rotated_translations(orientations, edges, rel)
    De = (d * d).sum(1) + 1.0
    ncol = 3 * m + E

    # A = [B; C] (SetupConstraintMatrix and the solver's constructor), duplicates summed as setFromTriplets does
    rows, cols, vals = [], [], []
    for e in range(E):
        for c in range(3):
            if ei[e] >= 0:
                rows.append(3 * e + c); cols.append(3 * ei[e] + c); vals.append(-1.0)
            if ej[e] >= 0:
                rows.append(3 * e + c); cols.append(3 * ej[e] + c); vals.append(1.0)
            rows.append(3 * e + c); cols.append(3 * m + e); vals.append(-d[e, c])
        rows.append(3 * E + e); cols.append(3 * m + e); vals.append(1.0)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(4 * E, ncol))
    b = np.concatenate([np.zeros(3 * E), np.ones(E)])

    full_solve = None
    if form == "full":
        full_solve = spla.factorized(sp.csc_matrix(A.T @ A))
    schur_cf = None
    if form == "schur" or check_schur:
        S = np.zeros((3 * m, 3 * m))
        M = np.eye(3)[None] - d[:, :, None] * d[:, None, :] / De[:, None, None]
        for e in range(E):
            a, c = ei[e], ej[e]
            for p, q, sgn in ((a, a, 1.0), (c, c, 1.0), (a, c, -1.0), (c, a, -1.0)):
                if p >= 0 and q >= 0:
                    S[3 * p:3 * p + 3, 3 * q:3 * q + 3] += sgn * M[e]
        schur_cf = sla.cho_factor(S, lower=True) if m else None

    def schur_solve(g):
        gp, gs = g[:3 * m].reshape(m, 3).copy(), g[3 * m:]
        h = d * (gs / De)[:, None]
        ok = ei >= 0
        np.add.at(gp, ei[ok], -h[ok])
        ok = ej >= 0
        np.add.at(gp, ej[ok], h[ok])
        xp = sla.cho_solve(schur_cf, gp.reshape(-1)).reshape(m, 3) if m else gp
        xi = np.where((ei >= 0)[:, None], xp[np.maximum(ei, 0)] if m else 0.0, 0.0)
        xj = np.where((ej >= 0)[:, None], xp[np.maximum(ej, 0)] if m else 0.0, 0.0)
        s = (gs - (d * (xi - xj)).sum(1)) / De
        return np.concatenate([xp.reshape(-1), s])

    out = dict(admm_iterations=0, converged=False, margins=[], schur_max_rel=0.0)
    z = np.zeros(4 * E)
    u = np.zeros(4 * E)
    x = np.zeros(ncol)
    rhs_norm = np.linalg.norm(b)
    p_abs = math.sqrt(4 * E) * o.absolute_tolerance
    d_abs = math.sqrt(ncol) * o.absolute_tolerance
    kappa = 1.0 / o.rho
    r_norm = s_norm = p_eps = d_eps = 0.0
    for _ in range(o.max_num_iterations):
        g = A.T @ (b + z - u)
        if form == "full":
            x = full_solve(g)
            if check_schur:
                xs = schur_solve(g)
                out["schur_max_rel"] = max(out["schur_max_rel"], np.abs(xs - x).max() / max(np.abs(x).max(), 1e-300))
        else:
            x = schur_solve(g)
        ax = A @ x
        ax_hat = o.alpha * ax + (1.0 - o.alpha) * (z + b)
        z_old = z
        v = ax_hat - b + u
        z = np.concatenate([np.maximum(0.0, v[:3 * E] - kappa) - np.maximum(0.0, -v[:3 * E] - kappa),
                            np.maximum(v[3 * E:], 0.0)])
        u = u + (ax_hat - z - b)
        r_norm = np.linalg.norm(ax - z - b)
        s_norm = np.linalg.norm(-o.rho * (A.T @ (z - z_old)))
        max_norm = max(np.linalg.norm(ax), np.linalg.norm(z), rhs_norm)
        p_eps = p_abs + o.relative_tolerance * max_norm
        d_eps = d_abs + o.relative_tolerance * np.linalg.norm(o.rho * (A.T @ u))
        out["admm_iterations"] += 1
        ok_r, ok_s = r_norm < p_eps, s_norm < d_eps
        mr, ms = _margin(r_norm, p_eps), _margin(s_norm, d_eps)
        if ok_r and ok_s:
            out["margins"].append(min(mr, ms))
            out["converged"] = True
            break
        out["margins"].append(max(mm for mm, ok in ((mr, ok_r), (ms, ok_s)) if not ok))
    pos = np.zeros((n, 3))
    pos[free] = x[:3 * m].reshape(m, 3)
    out.update(positions=pos, scales=x[3 * m:].copy(), final_margins=out["margins"][-2:], r_norm=float(r_norm),
               s_norm=float(s_norm), primal_eps=float(p_eps), dual_eps=float(d_eps),
               cpu_ms=1e3 * (time.perf_counter() - t0))
    return out
