"""numpy / scipy restatement of RobustRotationEstimator::EstimateRotations (global_pose_estimation/
robust_rotation_estimator.cc:66-294 with math/l1_solver.h:113-170 and math/rotation.cc:56-66), written from the
reference's description, line by line:

  residual   e_ij = MultiplyRotations(-r_j, MultiplyRotations(r_ij, r_i))                       (:268-284)
  update     r_i <- MultiplyRotations(r_i, delta_i), free views                                  (:252-266)
  step       mean over the free views of |delta_i|                                               (:286-294)
  L1         A'A factored once; <= max_num_l1_iterations ADMM solves (z = u = 0, rho = alpha = 1, tolerances 1e-4 / 1e-2),
             the iteration cap 5, 10, 20, ...; stop when step <= l1_step_convergence_threshold  (:164-185)
  IRLS       w = sigma / (|e|^2 + sigma^2)^2; solve A'WA d = A'W e; stop when step < irls threshold (:187-250)

The linear algebra uses A'WA = L_w (x) I_3 (one N x N Cholesky, three right-hand sides).  With check_kron=True every
solve is repeated in the reference's own form -- the 3E x 3N sparse A, A'WA as a 3N x 3N sparse product, a sparse
direct solve -- and the largest relative difference is recorded.  Every convergence decision records its margin:
how far (relative) the deciding comparisons sit from their thresholds."""
import math
import time

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

DBL_EPSILON = np.finfo(np.float64).eps


def aa_to_R(aa):
    """ceres::AngleAxisToRotationMatrix for rows of aa [n][3]; R [n][3][3]."""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    theta2 = np.einsum("ni,ni->n", aa, aa)
    big = theta2 > DBL_EPSILON
    theta = np.sqrt(np.where(big, theta2, 1.0))
    w = aa / theta[:, None]
    c, s = np.cos(theta), np.sin(theta)
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    R = np.empty((aa.shape[0], 3, 3))
    R[:, 0, 0] = c + wx * wx * (1 - c); R[:, 0, 1] = wx * wy * (1 - c) - wz * s; R[:, 0, 2] = wy * s + wx * wz * (1 - c)
    R[:, 1, 0] = wz * s + wx * wy * (1 - c); R[:, 1, 1] = c + wy * wy * (1 - c); R[:, 1, 2] = -wx * s + wy * wz * (1 - c)
    R[:, 2, 0] = -wy * s + wx * wz * (1 - c); R[:, 2, 1] = wx * s + wy * wz * (1 - c); R[:, 2, 2] = c + wz * wz * (1 - c)
    sm = ~big
    if sm.any():
        a = aa[sm]
        Rs = np.empty((a.shape[0], 3, 3))
        Rs[:, 0, 0] = 1.0; Rs[:, 0, 1] = -a[:, 2]; Rs[:, 0, 2] = a[:, 1]
        Rs[:, 1, 0] = a[:, 2]; Rs[:, 1, 1] = 1.0; Rs[:, 1, 2] = -a[:, 0]
        Rs[:, 2, 0] = -a[:, 1]; Rs[:, 2, 1] = a[:, 0]; Rs[:, 2, 2] = 1.0
        R[sm] = Rs
    return R


def R_to_aa(R):
    """ceres::RotationMatrixToAngleAxis (RotationMatrixToQuaternion, then QuaternionToAngleAxis) for R [n][3][3]."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    n = R.shape[0]
    q = np.empty((n, 4))
    trace = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    pos = trace >= 0.0
    if pos.any():
        Rp = R[pos]
        t = np.sqrt(trace[pos] + 1.0)
        q0 = 0.5 * t
        t = 0.5 / t
        q[pos] = np.stack([q0, (Rp[:, 2, 1] - Rp[:, 1, 2]) * t, (Rp[:, 0, 2] - Rp[:, 2, 0]) * t, (Rp[:, 1, 0] - Rp[:, 0, 1]) * t], 1)
    for r in np.nonzero(~pos)[0]:
        M = R[r]
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
        q[r, i + 1] = 0.5 * t
        t = 0.5 / t
        q[r, 0] = (M[k, j] - M[j, k]) * t
        q[r, j + 1] = (M[j, i] + M[i, j]) * t
        q[r, k + 1] = (M[k, i] + M[i, k]) * t
    s2 = q[:, 1] ** 2 + q[:, 2] ** 2 + q[:, 3] ** 2
    st = np.sqrt(s2)
    ct = q[:, 0]
    two_theta = 2.0 * np.where(ct < 0.0, np.arctan2(-st, -ct), np.arctan2(st, ct))
    k = np.where(s2 > 0.0, two_theta / np.where(s2 > 0.0, st, 1.0), 2.0)
    return q[:, 1:] * k[:, None]


def multiply_rotations(a, b):
    """MultiplyRotations (math/rotation.cc:56-66) row by row."""
    return R_to_aa(aa_to_R(a) @ aa_to_R(b))


class Options:   # robust_rotation_estimator.h:64-84
    def __init__(self, **kw):
        self.max_num_l1_iterations = 5
        self.l1_step_convergence_threshold = 0.001
        self.max_num_irls_iterations = 100
        self.irls_step_convergence_threshold = 0.001
        self.irls_loss_parameter_sigma = math.radians(5.0)
        for k, v in kw.items():
            setattr(self, k, v)


def _margin(value, threshold):
    return abs(value - threshold) / max(abs(threshold), 1e-300)


def robust_rotation_averaging(init, edges, rel, fixed=None, options=None, check_kron=False):
    """Returns a dict: orientations [n][3], l1_iterations, admm_iterations, irls_iterations, margins (every convergence
    decision: (kind, relative margin)), kron_max_rel (check_kron), final_squared_residual, cpu_ms."""
    t0 = time.perf_counter()
    o = options or Options()
    aa = np.array(init, dtype=np.float64).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    n, E = aa.shape[0], edges.shape[0]
    fix = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool).copy()
    if not fix.any():
        fix[0] = True
    idx = -np.ones(n, dtype=np.int64)
    free = np.nonzero(~fix)[0]
    m = len(free)
    idx[free] = np.arange(m)
    ei, ej = idx[edges[:, 0]], idx[edges[:, 1]]
    Rrel = aa_to_R(rel)
    out = dict(l1_iterations=0, admm_iterations=0, irls_iterations=0, margins=[], kron_max_rel=0.0)

    # A: one 3-row block per edge, -I at view i, +I at view j (SetupLinearSystem, :112-162), as a sparse matrix
    rows, cols, vals = [], [], []
    for e in range(E):
        for col, v in ((ei[e], -1.0), (ej[e], 1.0)):
            if col >= 0:
                for c in range(3):
                    rows.append(3 * e + c); cols.append(3 * col + c); vals.append(v)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(3 * E, 3 * m))   # duplicates summed, as setFromTriplets

    def residuals():
        t = R_to_aa(Rrel @ aa_to_R(aa[edges[:, 0]]))
        return R_to_aa(aa_to_R(-aa[edges[:, 1]]) @ aa_to_R(t))

    def At(v):       # A' v for v [E][3] -> [m][3]
        g = np.zeros((m, 3))
        ok = ei >= 0
        np.add.at(g, ei[ok], -v[ok])
        ok = ej >= 0
        np.add.at(g, ej[ok], v[ok])
        return g

    def Ax(x):       # A x for x [m][3] -> [E][3]
        xi = np.where((ei >= 0)[:, None], x[np.maximum(ei, 0)], 0.0)
        xj = np.where((ej >= 0)[:, None], x[np.maximum(ej, 0)], 0.0)
        return xj - xi

    def laplacian(w):   # L_w: A'WA = L_w (x) I_3
        Lw = np.zeros((m, m))
        for a, b in ((ei, ei), (ej, ej)):
            ok = a >= 0
            np.add.at(Lw, (a[ok], b[ok]), w[ok])
        ok = (ei >= 0) & (ej >= 0)
        np.add.at(Lw, (ei[ok], ej[ok]), -w[ok])
        np.add.at(Lw, (ej[ok], ei[ok]), -w[ok])
        return Lw

    def solve(cf, rhs, w):
        x = sla.cho_solve(cf, rhs)
        if check_kron:
            W = sp.diags(np.repeat(w, 3))
            big = spla.spsolve(sp.csc_matrix(A.T @ W @ A), rhs.reshape(-1))
            out["kron_max_rel"] = max(out["kron_max_rel"], np.abs(big - x.reshape(-1)).max() / np.abs(big).max())
        return x

    def update(x):
        aa[free] = multiply_rotations(aa[free], x)
        return np.linalg.norm(x, axis=1).sum() / m

    e = residuals()
    if m == 0:
        out.update(orientations=aa, final_squared_residual=float((e * e).sum()), cpu_ms=1e3 * (time.perf_counter() - t0))
        return out
    # ---- L1 (SolveL1Regression): L1Solver(A) factors A'A once
    ones = np.ones(E)
    cf = sla.cho_factor(laplacian(ones), lower=True)
    max_it = 5
    x = np.zeros((m, 3))
    for _ in range(o.max_num_l1_iterations):
        b = e.copy()
        z = np.zeros_like(b); u = np.zeros_like(b)
        rhs_norm = np.linalg.norm(b)
        p_abs = math.sqrt(3 * E) * 1e-4
        d_abs = math.sqrt(3 * m) * 1e-4
        for _ in range(max_it):
            x = solve(cf, At(b + z - u), ones)
            ax = Ax(x)
            ax_hat = ax                      # alpha = 1
            z_old = z
            v = ax_hat - b + u
            z = np.maximum(0.0, v - 1.0) - np.maximum(0.0, -v - 1.0)   # Shrinkage(., 1 / rho)
            u = u + (ax_hat - z - b)
            r_norm = np.linalg.norm(ax - z - b)
            s_norm = np.linalg.norm(-At(z - z_old))
            p_eps = p_abs + 1e-2 * max(np.linalg.norm(ax), np.linalg.norm(z), rhs_norm)
            d_eps = d_abs + 1e-2 * np.linalg.norm(At(u))
            out["admm_iterations"] += 1
            ok_r, ok_s = r_norm < p_eps, s_norm < d_eps
            mr, ms = _margin(r_norm, p_eps), _margin(s_norm, d_eps)
            if ok_r and ok_s:
                out["margins"].append(("admm", min(mr, ms)))
                break
            out["margins"].append(("admm", max(mm for mm, ok in ((mr, ok_r), (ms, ok_s)) if not ok)))
        step = update(x)
        e = residuals()
        out["l1_iterations"] += 1
        out["margins"].append(("l1", _margin(step, o.l1_step_convergence_threshold)))
        if step <= o.l1_step_convergence_threshold:
            break
        max_it *= 2
    # ---- IRLS (SolveIRLS)
    sigma = o.irls_loss_parameter_sigma
    for _ in range(o.max_num_irls_iterations):
        tmp = (e * e).sum(1) + sigma * sigma
        w = sigma / (tmp * tmp)
        cf = sla.cho_factor(laplacian(w), lower=True)
        x = solve(cf, At(w[:, None] * e), w)
        step = update(x)
        e = residuals()
        out["irls_iterations"] += 1
        out["margins"].append(("irls", _margin(step, o.irls_step_convergence_threshold)))
        if step < o.irls_step_convergence_threshold:
            break
    out.update(orientations=aa, final_squared_residual=float((e * e).sum()), cpu_ms=1e3 * (time.perf_counter() - t0))
    return out
