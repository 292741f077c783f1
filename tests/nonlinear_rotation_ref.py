"""An INDEPENDENT restatement of NonlinearRotationEstimator::EstimateRotations (global_pose_estimation/
nonlinear_rotation_estimator.cc:49-98, pairwise_rotation_error.h:65-96) for small view graphs, used to pin
theia_hip_nonlinear_rotations (csrc/nonlinear_rotations.hip):
  * the residual log(R(w2) R(w1)' R(rel)') written in torch (float64) with the branches of ceres::AngleAxisToRotationMatrix
    (theta^2 > eps: Rodrigues, else I + [w]x), RotationMatrixToQuaternion (trace >= 0, else the largest diagonal entry) and
    QuaternionToAngleAxis (sin^2 > 0: 2 atan2 / sin with the cos < 0 signs, else the factor 2), each branch selected by
    torch.where over inputs made safe for the branch not taken, and differentiated by torch.func (reverse mode) -- no
    code or derivation shared with the closed forms of csrc/;
  * SoftLOneLoss with Ceres' corrector for rho'' <= 0 (tests/independent_lm.py::loss);
  * the FULL dense normal equations and the trust-region rules of tests/independent_lm.py::solve (Ceres 2.2), with the
    solver options NonlinearRotationEstimator leaves at Ceres' defaults (max_trust_region_radius 1e16), a failed
    factorisation as an invalid step, held views, the trace, the step counts, the termination and the relative margin
    of every decision."""
import numpy as np
import torch
from torch.func import jacrev, vmap

from tests.independent_lm import loss

TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_CAP, TERM_FAILURE, TERM_RADIUS = 1, 2, 3, 4, 5, 6
EPS = float(np.finfo(np.float64).eps)


def _skew(w):
    z = torch.zeros_like(w[0])
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def _rot(w):
    t2 = (w * w).sum()
    big = t2 > EPS
    th = torch.sqrt(torch.where(big, t2, torch.ones_like(t2)))
    k = w / th
    K = _skew(k)
    eye = torch.eye(3, dtype=w.dtype)
    Rb = torch.cos(th) * eye + (1.0 - torch.cos(th)) * torch.outer(k, k) + torch.sin(th) * K
    return torch.where(big, Rb, eye + _skew(w))


def _log(E):
    tr = E[0, 0] + E[1, 1] + E[2, 2]
    d = torch.stack([E[0, 0], E[1, 1], E[2, 2]])
    i1 = d[1] > d[0]
    di = torch.where(i1, d[1], d[0])
    i2 = d[2] > di
    sel = [tr >= 0.0, (tr < 0.0) & ~i1 & ~i2, (tr < 0.0) & i1 & ~i2, (tr < 0.0) & i2]
    one = torch.ones_like(tr)
    qs = []
    t = torch.sqrt(torch.where(sel[0], tr + 1.0, one))
    qs.append(torch.stack([0.5 * t, (E[2, 1] - E[1, 2]) * (0.5 / t), (E[0, 2] - E[2, 0]) * (0.5 / t), (E[1, 0] - E[0, 1]) * (0.5 / t)]))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        t = torch.sqrt(torch.where(sel[1 + i], E[i, i] - E[j, j] - E[k, k] + 1.0, one))
        ent = [None] * 4
        ent[0] = (E[k, j] - E[j, k]) * (0.5 / t)
        ent[i + 1] = 0.5 * t
        ent[j + 1] = (E[j, i] + E[i, j]) * (0.5 / t)
        ent[k + 1] = (E[k, i] + E[i, k]) * (0.5 / t)
        qs.append(torch.stack(ent))
    q = torch.where(sel[0], qs[0], torch.where(sel[1], qs[1], torch.where(sel[2], qs[2], qs[3])))
    v = q[1:]
    s2 = (v * v).sum()
    has = s2 > 0.0
    st = torch.sqrt(torch.where(has, s2, one))
    two_theta = 2.0 * torch.where(q[0] < 0.0, torch.atan2(-st, -q[0]), torch.atan2(st, q[0]))
    return torch.where(has, v * (two_theta / st), v * 2.0)


def residual(w1, w2, rel):
    return _log(_rot(w2) @ _rot(w1).T @ _rot(rel).T)


_res = vmap(residual)
_jac = vmap(jacrev(residual, argnums=(0, 1)))


class Problem:
    def __init__(self, edges, rel, fixed, n, width):
        self.edges = np.asarray(edges).reshape(-1, 2)
        self.rel = torch.tensor(np.asarray(rel, dtype=np.float64).reshape(-1, 3))
        self.width = float(width)
        held = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        touched = np.zeros(n, dtype=bool)
        touched[self.edges.reshape(-1)] = True
        self.free = np.nonzero(touched & ~held)[0]                   # the views of the problem, in view order
        self.col = -np.ones(n, dtype=np.int64)
        self.col[self.free] = 3 * np.arange(len(self.free))
        # a residual whose two views are both held is not in the problem (Ceres removes it from the program)
        self.live = (self.col[self.edges[:, 0]] >= 0) | (self.col[self.edges[:, 1]] >= 0)
        self.n = 3 * len(self.free)

    def evaluate(self, x, jac):
        e = self.edges[self.live]
        w1, w2, rel = torch.tensor(x[e[:, 0]]), torch.tensor(x[e[:, 1]]), self.rel[torch.tensor(self.live)]
        r = _res(w1, w2, rel).numpy()
        s = (r * r).sum(1)
        rho, rho1 = loss("softl1", self.width, s)
        cost = 0.5 * float(rho.sum())
        sr = np.sqrt(rho1)
        rc = (r * sr[:, None]).reshape(-1)
        if not jac:
            return cost, rc, None
        j1, j2 = (t.numpy() for t in _jac(w1, w2, rel))
        J = np.zeros((len(rc), self.n))
        for k in range(len(e)):
            c1, c2 = self.col[e[k, 0]], self.col[e[k, 1]]
            if c1 >= 0:
                J[3 * k:3 * k + 3, c1:c1 + 3] = sr[k] * j1[k]
            if c2 >= 0:
                J[3 * k:3 * k + 3, c2:c2 + 3] = sr[k] * j2[k]
        return cost, rc, J

    def plus(self, x, delta):
        x = x.copy()
        x[self.free] += delta.reshape(-1, 3)
        return x

    def norm(self, x, x2=None):
        d = x[self.free] - (x2[self.free] if x2 is not None else 0.0)
        return float(np.sqrt((d * d).sum()))


def _margin(a, b):
    """relative distance of the two sides of a comparison"""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0.0 else 1.0


def solve(orientations, edges, rel, fixed=None, robust_loss_width=0.1, max_num_iterations=200, function_tolerance=1e-6,
          gradient_tolerance=1e-10, parameter_tolerance=1e-8, max_trust_region_radius=1e16, linear="cholesky"):
    """Returns a dict: x (orientations, the input after a FAILURE), trace [(cost, gradient max norm, step norm, radius,
    accepted)], iterations, successful, unsuccessful, invalid, term, margin (the smallest relative margin of a decision),
    step_norms / x_norms / gmaxs (per pass, for the tests that place a tolerance between two of them)."""
    x0 = np.array(orientations, dtype=np.float64).reshape(-1, 3)
    P = Problem(edges, rel, fixed, x0.shape[0], robust_loss_width)
    x = x0.copy()
    x_cost, r, J = P.evaluate(x, True)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    gmax = float(np.abs(J.T @ r).max())
    x_norm = P.norm(x)
    radius, decrease = 1e4, 2.0
    trace = [(x_cost, gmax, 0.0, radius, 1)]
    out = dict(iterations=0, successful=0, unsuccessful=0, invalid=0, margin=np.inf, step_norms=[], x_norms=[x_norm], gmaxs=[gmax])
    it, invalid_run, successful, term = 0, 0, True, None

    def decide(a, b):
        out["margin"] = min(out["margin"], _margin(a, b))

    decide(gmax, gradient_tolerance)
    if gmax <= gradient_tolerance:
        term = TERM_GRADIENT
    while term is None:
        if it >= max_num_iterations:
            term = TERM_CAP; break
        if successful:
            decide(gmax, gradient_tolerance)
            if gmax <= gradient_tolerance:
                term = TERM_GRADIENT; break
        if radius <= 1e-32:
            term = TERM_RADIUS; break
        it += 1
        D2 = np.clip((Js * Js).sum(0), 1e-6, 1e32) / radius
        A = Js.T @ Js + np.diag(D2)
        try:
            if linear == "lu":
                y = np.linalg.solve(A, Js.T @ r)
            else:
                Lc = np.linalg.cholesky(A)
                y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Js.T @ r))
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            ok = False
        mcc = 0.0
        if ok:
            m = Js @ (-y)
            mcc = -float(m @ (r + m / 2.0))
            ok = mcc > 0.0
        if not ok:
            out["invalid"] += 1
            invalid_run += 1
            if invalid_run >= 5:
                term = TERM_FAILURE; break
            radius /= decrease; decrease *= 2.0; successful = False
            trace.append((x_cost, gmax, 0.0, radius, 0))
            continue
        invalid_run = 0
        xc = P.plus(x, -y * scale)
        cand, rc, _ = P.evaluate(xc, False)
        if not np.all(np.isfinite(rc)):
            cand = np.finfo(np.float64).max
        step_norm = P.norm(x, xc)
        out["step_norms"].append(step_norm)
        decide(step_norm, parameter_tolerance * (x_norm + parameter_tolerance))
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            trace.append((cand, gmax, step_norm, radius, 0)); term = TERM_PARAMETER; break
        change = x_cost - cand
        decide(abs(change), function_tolerance * x_cost)
        if abs(change) <= function_tolerance * x_cost:
            trace.append((cand, gmax, step_norm, radius, 0)); term = TERM_FUNCTION; break
        rho = change / mcc
        decide(rho, 1e-3)
        if rho > 1e-3:
            x = xc
            x_norm = P.norm(x)
            x_cost, r, J = P.evaluate(x, True)
            Js = J * scale
            gmax = float(np.abs(J.T @ r).max())
            radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease = 2.0; successful = True
            out["successful"] += 1
            out["x_norms"].append(x_norm); out["gmaxs"].append(gmax)
            trace.append((x_cost, gmax, step_norm, radius, 1))
        else:
            radius /= decrease; decrease *= 2.0; successful = False
            out["unsuccessful"] += 1
            trace.append((cand, gmax, step_norm, radius, 0))
    out.update(x=x0 if term == TERM_FAILURE else x, trace=trace, iterations=it, term=term, radius=radius, cost=x_cost,
               initial_cost=trace[0][0])
    return out
