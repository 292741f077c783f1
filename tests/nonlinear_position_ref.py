"""An INDEPENDENT restatement of NonlinearPositionEstimator::EstimatePositions (global_pose_estimation/
nonlinear_position_estimator.cc:136-206, pairwise_translation_error.h:65-100) for small problems, used to pin
theia_hip_nonlinear_positions (csrc/nonlinear_positions.hip):
  * the residual written in torch (float64): w (d - s t) where the edge has a scale estimate, else w (d / |d| - t) with the
    norm replaced by the constant 1 below 1e-12, each branch selected by torch.where over inputs made safe for the branch
    not taken, and differentiated by torch.func (reverse mode) -- no code or derivation shared with the closed forms of
    csrc/;
  * the directions R(w)' position_2 and normalize(R(w_ray)' [x, y, 1]) through the torch rotation of
    tests/nonlinear_rotation_ref.py (ceres::AngleAxisToRotationMatrix with its small-angle branch);
  * HuberLoss with Ceres' corrector for rho'' <= 0 (tests/independent_lm.py::loss);
  * the FULL dense normal equations with the track points as unknowns beside the views, and the trust-region rules of
    Ceres 2.2 as tests/nonlinear_rotation_ref.py states them: a failed factorisation as an invalid step, held views, the
    trace, the step counts, the termination and the relative margin of every decision; solved by Cholesky or, on
    request, by LU."""
import numpy as np
import torch
from torch.func import jacrev, vmap

from tests.independent_lm import loss
from tests.nonlinear_rotation_ref import _rot

TERM_NONE, TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_CAP, TERM_FAILURE, TERM_RADIUS = 0, 1, 2, 3, 4, 5, 6
NORM_TOLERANCE = 1e-12


def residual(xa, xb, t, w, s):
    d = xb - xa
    n2 = (d * d).sum()
    one = torch.ones_like(n2)
    nrm = torch.sqrt(torch.where(n2 > 0.0, n2, one))
    tiny = torch.where(n2 > 0.0, nrm, torch.zeros_like(n2)) < NORM_TOLERANCE
    nrm = torch.where(tiny, one, nrm)               # the constant 1: no derivative
    return torch.where(s > 0.0, w * (d - s * t), w * (d / nrm - t))


_res = vmap(residual)
_jac = vmap(jacrev(residual, argnums=(0, 1)))


def rotated(w, v):
    """R(w)' v for rows of angle-axis vectors w and vectors v."""
    return np.array([(_rot(torch.tensor(a)).T @ torch.tensor(b)).numpy() for a, b in zip(np.asarray(w, dtype=np.float64),
                                                                                     np.asarray(v, dtype=np.float64))]).reshape(-1, 3)


class Problem:
    """Nodes: the n views, then the T points.  Edges: the pairs in input order, then one per observation (view -> point)."""

    def __init__(self, orientations, edges, rel, scales, fixed, points, track_offsets, obs_view, obs_feature,
                 ray_orientations, weight, width):
        aa = np.asarray(orientations, dtype=np.float64).reshape(-1, 3)
        n = self.n_views = aa.shape[0]
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
        Ec = len(e)
        t = rotated(aa[e[:, 0]], rel)
        w = np.ones(Ec)
        s = -np.ones(Ec) if scales is None else np.asarray(scales, dtype=np.float64).reshape(-1)
        T = 0 if points is None else len(points)
        if T:
            off = np.asarray(track_offsets, dtype=np.int64)
            ov = np.asarray(obs_view, dtype=np.int64)
            of = np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2)
            ray_aa = aa if ray_orientations is None else np.asarray(ray_orientations, dtype=np.float64).reshape(-1, 3)
            track = np.repeat(np.arange(T), np.diff(off))
            rays = rotated(ray_aa[ov], np.column_stack([of, np.ones(len(of))]))
            rays /= np.linalg.norm(rays, axis=1, keepdims=True)
            e = np.concatenate([e, np.column_stack([ov, n + track])])
            t = np.concatenate([t, rays]); w = np.concatenate([w, np.full(len(ov), float(weight))])
            s = np.concatenate([s, -np.ones(len(ov))])
        self.edges, self.num_camera_edges = e, Ec
        self.t, self.w, self.s = torch.tensor(t), torch.tensor(w), torch.tensor(s)
        self.width = float(width)
        N = self.N = n + T
        held = np.zeros(N, dtype=bool)
        if fixed is not None:
            held[:n] = np.asarray(fixed, dtype=bool)
        touched = np.zeros(N, dtype=bool)
        touched[e.reshape(-1)] = True
        self.free = np.nonzero(touched & ~held)[0]
        self.col = -np.ones(N, dtype=np.int64)
        self.col[self.free] = 3 * np.arange(len(self.free))
        # a residual whose two nodes are both held is not in the problem (Ceres removes it from the program)
        self.live = (self.col[e[:, 0]] >= 0) | (self.col[e[:, 1]] >= 0)
        self.n = 3 * len(self.free)
        self.seen = dict(inlier=False, outlier=False, scaled=False, normalised=False, tiny=False)

    def evaluate(self, x, jac):
        lv = torch.tensor(self.live)
        e = self.edges[self.live]
        xa, xb = torch.tensor(x[e[:, 0]]), torch.tensor(x[e[:, 1]])
        t, w, s = self.t[lv], self.w[lv], self.s[lv]
        r = _res(xa, xb, t, w, s).numpy()
        q = (r * r).sum(1)
        rho, rho1 = loss("huber", self.width, q)
        cost = 0.5 * float(rho.sum())
        sr = np.sqrt(rho1)
        rc = (r * sr[:, None]).reshape(-1)
        if not jac:
            return cost, rc, None
        dist = np.linalg.norm(x[e[:, 1]] - x[e[:, 0]], axis=1)
        scaled = s.numpy() > 0.0
        self.seen["inlier"] |= bool((q <= self.width ** 2).any()); self.seen["outlier"] |= bool((q > self.width ** 2).any())
        self.seen["scaled"] |= bool(scaled.any()); self.seen["tiny"] |= bool((~scaled & (dist < NORM_TOLERANCE)).any())
        self.seen["normalised"] |= bool((~scaled & (dist >= NORM_TOLERANCE)).any())
        j1, j2 = (v.numpy() for v in _jac(xa, xb, t, w, s))
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


def solve(orientations, positions, edges, rel, scales=None, fixed=None, points=None, track_offsets=None, obs_view=None,
          obs_feature=None, ray_orientations=None, point_to_camera_weight=0.5, robust_loss_width=0.1,
          max_num_iterations=400, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
          max_trust_region_radius=1e16, linear="cholesky"):
    """Returns a dict: x (positions) and points (the input after a FAILURE), trace [(cost, gradient max norm, step norm,
    radius, accepted)], iterations, successful, unsuccessful, invalid, term, margin (the smallest relative margin of a
    decision), step_norms / x_norms / gmaxs (per pass, for the tests that place a tolerance between two of them), seen
    (which residual branches and Huber regions a linearisation met), order (of the dense system)."""
    p0 = np.array(positions, dtype=np.float64).reshape(-1, 3)
    n = p0.shape[0]
    x0 = p0 if points is None else np.concatenate([p0, np.array(points, dtype=np.float64).reshape(-1, 3)])
    P = Problem(orientations, edges, rel, scales, fixed, points, track_offsets, obs_view, obs_feature, ray_orientations,
                point_to_camera_weight, robust_loss_width)
    out = dict(iterations=0, successful=0, unsuccessful=0, invalid=0, margin=np.inf, step_norms=[], x_norms=[], gmaxs=[],
               order=P.n, seen=P.seen)
    if P.n == 0:
        out.update(x=p0, points=x0[n:], trace=[], term=TERM_NONE, radius=0.0, cost=0.0, initial_cost=0.0)
        return out
    x = x0.copy()
    x_cost, r, J = P.evaluate(x, True)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    gmax = float(np.abs(J.T @ r).max())
    x_norm = P.norm(x)
    radius, decrease = 1e4, 2.0
    trace = [(x_cost, gmax, 0.0, radius, 1)]
    out["x_norms"].append(x_norm); out["gmaxs"].append(gmax)
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
    final = x0 if term == TERM_FAILURE else x
    out.update(x=final[:n], points=final[n:], trace=trace, iterations=it, term=term, radius=radius, cost=x_cost,
               initial_cost=trace[0][0])
    return out
