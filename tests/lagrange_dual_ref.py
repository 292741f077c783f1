"""numpy restatement of LagrangeDualRotationEstimator::EstimateRotations with its default solver, written from the
reference's description, line by line (global_pose_estimation/lagrange_dual_rotation_estimator.cc:51-197,
math/rank_restricted_sdp_solver.cc:58-129, math/riemannian_staircase.cc:57-111 and :113-319, math/bcm_sdp_solver.h:64-72,
math/rotation.cc:105-120):

  setup      e = (i, j), R_e = AngleAxisToRotationMatrix(rotation_2): R has R_e' at block (i, j), R_e at block (j, i);
             Q = -R; Y [r][3n] starts at zero
  sweep      G = Y Q once; for i = 0 .. n-1: Y_i = U V' of the thin SVD of -G_i ([I_3; 0] for a zero block, what Eigen's
             JacobiSVD returns there); G_j += (Y_i - old Y_i) Q_ij for the neighbours j          (sequential, incremental)
  stopping   before each sweep err = |f_prev - f| / max(|f_prev|, 1), f_prev = DBL_MAX at first; stop when err <= tol
             or after max_iterations sweeps; total_iterations_num = sweeps + 1
  staircase  for r = min_rank .. max_rank: the BCM; Lambda = SymBlockDiag(Q Y' Y); lambda_min(Q - Lambda) (eigh here, the
             reference's Lanczos starts from a random vector); > -tolerance: stop; else a zero row under Y, Ydot = its
             last row v_min', alpha from max(16e-6, 10 gtol / |lambda_min|) halved down to 1e-6, the first trial
             polar(Y + alpha Ydot) with f < f(Y), |grad| > gtol and |grad| > pgtol, else the trial of least f when below
             f(Y), else stop
  solution   X_i = Y_0' Y_i, ProjectToSOd when the rank left behind is above min_rank; orientation = X_i', negated when
             its determinant is negative, as angle-axis

Besides the literal sums (`sums="incremental"`) the sweep can gather G_i afresh at every update with the neighbours in
ascending or descending order: the difference between those two is the arithmetic's own noise, which the GPU tests take
their tolerance from.  `order` relabels the sweep (the reference's SetViewIdToIndex allows exactly this).  Every stopping
and certificate decision and the smallest singular value ratio met are recorded for the fairness checks."""
import math

import numpy as np

from tests.rotation_averaging_ref import aa_to_R, R_to_aa

DBL_MAX = np.finfo(np.float64).max


class Options:   # math/solver_options.h:44-97
    def __init__(self, **kw):
        self.max_iterations = 500
        self.tolerance = 1e-8
        self.min_rank = 3
        self.max_rank = 10
        self.min_eigenvalue_nonnegativity_tolerance = 1e-5
        self.gradient_tolerance = 1e-2
        self.preconditioned_gradient_tolerance = 1e-4
        for k, v in kw.items():
            setattr(self, k, v)


def build_problem(n, edges, rel):
    """Q (dense 3n x 3n) and the neighbour lists in ascending order.  Views are those of 0 .. n-1."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    Re = aa_to_R(rel)
    R = np.zeros((3 * n, 3 * n))
    adj = [[] for _ in range(n)]
    for e, (i, j) in enumerate(edges):
        R[3 * i:3 * i + 3, 3 * j:3 * j + 3] = Re[e].T
        R[3 * j:3 * j + 3, 3 * i:3 * i + 3] = Re[e]
        adj[i].append(int(j)); adj[j].append(int(i))
    return -R, [sorted(a) for a in adj]


def polar(A):
    """U V' of the thin SVD; [I_3; 0] for a zero block.  Also returns sigma_min (inf for a zero block)."""
    if not A.any():
        return np.eye(A.shape[0], 3), math.inf
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    return U @ Vt, s[-1]


def fval(Q, Y):
    return float(np.trace(Y @ (Q @ Y.T)))


def greedy_colour_order(adj):
    """Views by (greedy colour in index order, index); the number of colours."""
    n = len(adj)
    colour = [-1] * n
    for i in range(n):
        used = {colour[j] for j in adj[i] if colour[j] >= 0}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return sorted(range(n), key=lambda v: (colour[v], v)), max(colour) + 1


def bcm(Q, adj, Y, opts, order=None, sums="incremental", record=None):
    """One block coordinate minimisation from Y [r][3n].  Returns (Y, sweeps, f).  record: dict that collects errs (the
    err of every stopping test) and min_sigma, the smallest singular value of any G_i that was factored."""
    n = len(adj)
    order = list(range(n)) if order is None else list(order)
    Y = Y.copy()
    blk = lambda i: slice(3 * i, 3 * i + 3)
    G = np.zeros_like(Y)
    for i in range(n):
        for j in adj[i]:
            G[:, blk(i)] += Y[:, blk(j)] @ Q[blk(j), blk(i)]
    f_prev, f_cur = DBL_MAX, fval(Q, Y)
    sweeps, errs, min_ratio = 0, [], math.inf
    while sweeps < opts.max_iterations:
        err = abs(f_prev - f_cur) / max(abs(f_prev), 1.0)
        errs.append(err)
        if err <= opts.tolerance:
            break
        for i in order:
            if sums == "incremental":
                Gi = G[:, blk(i)].copy()
            else:
                Gi = np.zeros((Y.shape[0], 3))
                for j in (adj[i] if sums == "ascending" else adj[i][::-1]):
                    Gi += Y[:, blk(j)] @ Q[blk(j), blk(i)]
            prev = Y[:, blk(i)].copy()
            Y[:, blk(i)], ratio = polar(-Gi)
            min_ratio = min(min_ratio, ratio)
            if sums == "incremental":
                for j in adj[i]:
                    G[:, blk(j)] += (Y[:, blk(i)] - prev) @ Q[blk(i), blk(j)]
        sweeps += 1
        f_prev, f_cur = f_cur, fval(Q, Y)
    if record is not None:
        record.setdefault("errs", []).append(errs)
        record["min_sigma"] = min(record.get("min_sigma", math.inf), min_ratio)
    return Y, sweeps, f_cur


def lambda_blocks(Q, Y):
    """Lambda [3][3n] = SymBlockDiag(Q Y' Y)."""
    n = Y.shape[1] // 3
    QYt = Q @ Y.T
    L = np.zeros((3, 3 * n))
    for i in range(n):
        P = QYt[3 * i:3 * i + 3] @ Y[:, 3 * i:3 * i + 3]
        L[:, 3 * i:3 * i + 3] = 0.5 * (P + P.T)
    return L


def certificate_matrix(Q, Y):
    S = Q.copy()
    L = lambda_blocks(Q, Y)
    for i in range(Y.shape[1] // 3):
        S[3 * i:3 * i + 3, 3 * i:3 * i + 3] -= L[:, 3 * i:3 * i + 3]
    return S


def project_blocks(A):
    n = A.shape[1] // 3
    P = np.empty_like(A)
    for i in range(n):
        P[:, 3 * i:3 * i + 3] = polar(A[:, 3 * i:3 * i + 3])[0]
    return P


def riemannian_gradient(Q, Y):
    n = Y.shape[1] // 3
    E = 2.0 * (Q @ Y.T).T
    out = np.empty_like(Y)
    for i in range(n):
        b = slice(3 * i, 3 * i + 3)
        P = Y[:, b].T @ E[:, b]
        out[:, b] = E[:, b] - Y[:, b] @ (0.5 * (P + P.T))
    return out


def escape_saddle(Q, Y_aug, lambda_min, v, opts):
    """Returns (Y+, alpha, fallback) or None."""
    FY = fval(Q, Y_aug)
    Ydot = np.zeros_like(Y_aug)
    Ydot[-1] = v
    alpha_min = 1e-6
    alpha = max(16 * alpha_min, 10 * opts.gradient_tolerance / abs(lambda_min))
    alphas, fvals = [], []
    while alpha >= alpha_min:
        Yt = project_blocks(Y_aug + alpha * Ydot)
        Ft = fval(Q, Yt)
        g = np.linalg.norm(riemannian_gradient(Q, Yt))
        alphas.append(alpha); fvals.append(Ft)
        if Ft < FY and g > opts.gradient_tolerance and g > opts.preconditioned_gradient_tolerance:
            return Yt, alpha, False
        alpha /= 2
    k = int(np.argmin(fvals))
    if fvals[k] < FY:
        return project_blocks(Y_aug + alphas[k] * Ydot), alphas[k], True
    return None


def admissible_direction(w, V, variant):
    """A unit v with v' S v <= 0.9 lambda_min from the eigenpairs of S: the eigenvector itself (variant 0), or it tilted by
    0.2 of the next one (variant 1)."""
    v = V[:, 0].copy()
    if variant == 1:
        v = v + 0.2 * V[:, 1]
        v /= np.linalg.norm(v)
        assert (w[0] + 0.04 * w[1]) / 1.04 <= 0.9 * w[0]
    k = int(np.argmax(np.abs(v)))
    return v if v[k] > 0 else -v


def project_to_sod(M):
    U, _, Vt = np.linalg.svd(M)
    if np.linalg.det(U) * np.linalg.det(Vt) > 0:
        return U @ Vt
    U = U.copy()
    U[:, -1] *= -1
    return U @ Vt


def solution(Y, rounded):
    """X [3][3n] with X_i = Y_0' Y_i (projected when `rounded`), and the orientations [n][3]."""
    n = Y.shape[1] // 3
    X = Y[:, :3].T @ Y
    aa = np.zeros((n, 3))
    for i in range(n):
        B = X[:, 3 * i:3 * i + 3]
        if rounded:
            B = project_to_sod(B)
            X[:, 3 * i:3 * i + 3] = B
        R = B.T
        if np.linalg.det(R) < 0:
            R = -R
        aa[i] = R_to_aa(R[None])[0]
    return X, aa


def solve(n, edges, rel, opts=None, staircase=True, y_init=None, order=None, sums="incremental", v_variant=0):
    """The estimator on the views 0 .. n-1, all of which have an edge.  Returns a dict: Y, X, orientations, f, final_rank,
    end ("bcm", "certified", "max_rank", "escape_failed"), total_iterations_num, levels (rank, sweeps, f, certified,
    lambda_min, alpha, fallback), record (errs per BCM, min_sigma)."""
    o = opts or Options()
    Q, adj = build_problem(n, edges, rel)
    rec = {}
    Y = np.zeros((o.min_rank if staircase else 3, 3 * n)) if y_init is None else np.array(y_init, dtype=np.float64)
    levels = []
    if not staircase:
        Y, sweeps, f = bcm(Q, adj, Y, o, order, sums, rec)
        levels.append(dict(rank=Y.shape[0], sweeps=sweeps, f=f, certified=False, lambda_min=math.nan, alpha=0.0, fallback=False))
        X, aa = solution(Y, Y.shape[0] > 3)
        return dict(Y=Y, X=X, orientations=aa, f=f, final_rank=Y.shape[0], end="bcm", total_iterations_num=sweeps + 1,
                    levels=levels, record=rec)
    end = "max_rank"
    r = Y.shape[0]
    while r <= o.max_rank:
        Y, sweeps, f = bcm(Q, adj, Y, o, order, sums, rec)
        S = certificate_matrix(Q, Y)
        w, V = np.linalg.eigh(S)
        lam = float(w[0])
        lv = dict(rank=r, sweeps=sweeps, f=f, certified=lam > -o.min_eigenvalue_nonnegativity_tolerance, lambda_min=lam,
                  alpha=0.0, fallback=False)
        levels.append(lv)
        if lv["certified"]:
            end = "certified"
            break
        Y = np.vstack([Y, np.zeros((1, 3 * n))])
        esc = escape_saddle(Q, Y, lam, admissible_direction(w, V, v_variant), o)
        if esc is None:
            end = "escape_failed"
            break
        Y, lv["alpha"], lv["fallback"] = esc
        r += 1
    X, aa = solution(Y, Y.shape[0] > o.min_rank)
    return dict(Y=Y, X=X, orientations=aa, f=fval(Q, Y), final_rank=Y.shape[0], end=end, total_iterations_num=sweeps + 1,
                levels=levels, record=rec)


def irls_refine(orientations, edges, rel, gauge=0):
    """HybridRotationEstimator's second half (hybrid_rotation_estimator.cc:69-109, irls_rotation_local_refiner.cc:77-160):
    IRLS only, 10 iterations, step threshold 1e-3, sigma = 5 degrees, the gauge view held."""
    from tests import rotation_averaging_ref as rar
    o = rar.Options(max_num_l1_iterations=0, max_num_irls_iterations=10, irls_step_convergence_threshold=1e-3,
                    irls_loss_parameter_sigma=math.radians(5.0))
    fixed = np.zeros(len(orientations), dtype=bool)
    fixed[gauge] = True
    return rar.robust_rotation_averaging(orientations, edges, rel, fixed, o)
