"""An INDEPENDENT first LM step of the three two-view refinements of csrc/twoview_lm.hip (BundleAdjustTwoViewsAngular,
OptimizeHomography, OptimizeFundamentalMatrix: bundle_adjust_two_views.cc:189-358), used by tests/test_twoview_edge_scenes*.py.
It shares no code or derivation with oracle/ (forward-mode Jets, closed-form manifold Jacobians) or csrc/ (closed forms):
  * the residuals are written from their definitions in torch float64 and differentiated by reverse-mode autodiff:
      - the angular epipolar error (angular_epipolar_error.h:54-91), the rotation as matrix_exp of the skew matrix;
      - the symmetric transfer error of a homography (homography_error.h:45-95), with torch.linalg.inv;
      - the squared Sampson distance as one residual (sampson_error.h:21-33);
  * the manifolds are written from their definitions:
      - ceres::SphereManifold<3>: x (+) d = |x| H(x)^T [sin|d| d / |d|; cos|d|] with the Householder reflection H(x) x = |x| e_3,
        its Jacobian the first two columns of |x| H(x)^T;
      - the fundamental-matrix manifold (fundamental_matrix_parameterization.h:15-75): with F = U diag(s) V^T from
        numpy.linalg.svd, Plus(F, d) = (U R(d[0:3])) diag(1, s1 / s0 + d[6], 0) (V R(d[3:6]))^T, its Jacobian by autodiff at d = 0;
  * the step rules are those of tests/independent_lm.py (jacobi_scale, trial_step, tolerance_stop, step_accepted), imported.
Three places follow Ceres and not smoothness:
  * a clamped angular residual (the square root's argument negative) is the constant 1000: its Jacobian row is zero;
  * ceres::AngleAxisToRotationMatrix is I + [w]x at theta^2 <= DBL_EPSILON, and that expression is what gets differentiated
    (for the pose and for the two rotations of the F manifold, which are always differentiated at d = 0);
  * likewise the Householder vector takes its x ~ +-e_3 branch at x0^2 + x1^2 <= DBL_EPSILON (beta = 0 or 2), where the
    reflection it stands for is only approximately the one of the definition.
A tangent basis of the F manifold is unique up to signs only while the singular values of F are distinct (the signs cancel in
the step); where they are not, numpy's SVD and another one span different bases and the Jacobi-scaled LM step differs."""
import numpy as np
import torch
from torch.func import jacrev

from tests import independent_lm as ilm

EPS = float(np.finfo(np.float64).eps)
TRIVIAL, HUBER, TRUNCATED = 0, 1, 6                       # theia_hip.h's loss_function_type
_LOSS = {TRIVIAL: "trivial", HUBER: "huber", TRUNCATED: "truncated"}


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


def _skew(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def _rotation(w, first_order):
    return torch.eye(3, dtype=w.dtype) + _skew(w) if first_order else torch.linalg.matrix_exp(_skew(w))


# ------------------------------------------------------------------ residuals
def _angular_terms(x, corr, first_order):
    R = _rotation(x[:3], first_order)
    t = x[3:]
    ones = torch.ones(corr.shape[0], 1, dtype=corr.dtype)
    f1 = torch.cat([corr[:, :2], ones], 1)
    f2 = torch.cat([corr[:, 2:], ones], 1)
    M = torch.eye(3, dtype=x.dtype) - torch.outer(t, t)
    u, w = f2 @ R.T, f2 @ R                                # R f2, R^T f2
    a = ((f1 @ M) * f1).sum(1) + ((w @ M.T) * u).sum(1)    # f1.(M f1) + (R f2).(M R^T f2)
    b = (torch.linalg.cross(f1, w) * t).sum(1)
    return a, a * a / 4.0 - b * b


def angular_residuals(x, corr, clamped=None):
    """[n] residuals at x = rotation (angle-axis) | position; clamped: the mask of the constant-1000 residuals (evaluated at x
    when None)."""
    first_order = float(x[:3].detach() @ x[:3].detach()) <= EPS
    if clamped is None:
        with torch.no_grad():
            clamped = _angular_terms(x, corr, first_order)[1] < 0.0
    a, s = _angular_terms(x, corr, first_order)
    r = a / 2.0 - torch.sqrt(torch.where(clamped, torch.ones_like(s), s))
    return torch.where(clamped, torch.full_like(r, 1000.0), r)


def homography_residuals(H, corr):
    """[n][4]: H x1 - x2 and H^-1 x2 - x1, dehomogenised; H 3 x 3"""
    ones = torch.ones(corr.shape[0], 1, dtype=corr.dtype)
    x1 = torch.cat([corr[:, :2], ones], 1)
    x2 = torch.cat([corr[:, 2:], ones], 1)
    p = x1 @ H.T
    q = x2 @ torch.linalg.inv(H).T
    return torch.cat([p[:, :2] / p[:, 2:] - corr[:, 2:], q[:, :2] / q[:, 2:] - corr[:, :2]], 1)


def sampson_residuals(F, corr):
    """[n]: (x2' F x1)^2 / ((F x1)_0^2 + (F x1)_1^2 + (F' x2)_0^2 + (F' x2)_1^2)"""
    ones = torch.ones(corr.shape[0], 1, dtype=corr.dtype)
    x1 = torch.cat([corr[:, :2], ones], 1)
    x2 = torch.cat([corr[:, 2:], ones], 1)
    Fx1 = x1 @ F.T
    Ftx2 = x2 @ F
    return (x2 * Fx1).sum(1) ** 2 / (Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2)


# ------------------------------------------------------------------ manifolds
def householder3(x):
    """v (v_2 = 1), beta of ceres' ComputeHouseholderVector: (I - beta v v') x = |x| e_3"""
    sigma = x[0] * x[0] + x[1] * x[1]
    v = np.array([x[0], x[1], 1.0])
    if sigma <= EPS:
        return v, (2.0 if x[2] < 0.0 else 0.0)
    mu = np.sqrt(x[2] * x[2] + sigma)
    vp = x[2] - mu if x[2] <= 0.0 else -sigma / (x[2] + mu)
    v[:2] /= vp
    return v, 2.0 * vp * vp / (sigma + vp * vp)


def sphere3_plus(x, d):
    nd = np.linalg.norm(d)
    if nd == 0.0:
        return x.copy()
    v, beta = householder3(x)
    y = np.append(np.sin(nd) / nd * d, np.cos(nd))
    return np.linalg.norm(x) * (y - v * (beta * (v @ y)))


def sphere3_plus_jacobian(x):
    v, beta = householder3(x)
    return np.linalg.norm(x) * (np.eye(3) - beta * np.outer(v, v))[:, :2]


def _fund_compose(U, V, ratio, d, first_order):
    Un = U @ _rotation(d[:3], first_order[0])
    Vn = V @ _rotation(d[3:6], first_order[1])
    return torch.outer(Un[:, 0], Vn[:, 0]) + (ratio + d[6]) * torch.outer(Un[:, 1], Vn[:, 1])


def fund_plus(F, d):
    U, S, Vt = np.linalg.svd(np.asarray(F, dtype=np.float64).reshape(3, 3))
    d = np.asarray(d, dtype=np.float64)
    fo = (float(d[:3] @ d[:3]) <= EPS, float(d[3:6] @ d[3:6]) <= EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = S[1] / S[0]
    return _fund_compose(_t(U), _t(Vt.T), _t(ratio), _t(d), fo).numpy()


def fund_plus_jacobian(F):
    """[9][7]: d vec(Plus(F, d)) / d d at d = 0 (row-major vec)"""
    U, S, Vt = np.linalg.svd(np.asarray(F, dtype=np.float64).reshape(3, 3))
    J = jacrev(lambda d: _fund_compose(_t(U), _t(Vt.T), _t(S[1] / S[0]), d, (True, True)).reshape(9))(torch.zeros(7, dtype=torch.float64))
    return J.numpy()


# ------------------------------------------------------------------ the three problems: evaluate(x, jac) and plus(x, d)
class Angular:
    """x = [6]; tangent = rotation (3) | sphere (2)"""
    def __init__(self, corr, loss_type, loss_width):
        self.corr, self.loss, self.width = _t(corr).reshape(-1, 4), _LOSS[loss_type], loss_width

    def raw(self, x):
        return angular_residuals(_t(x), self.corr).numpy().reshape(-1, 1)

    def evaluate(self, x, jac):
        r = self.raw(x)
        if not jac:
            return r, None
        xt = _t(x)
        with torch.no_grad():
            clamped = _angular_terms(xt, self.corr, float(xt[:3] @ xt[:3]) <= EPS)[1] < 0.0
        Ja = jacrev(lambda z: angular_residuals(z, self.corr, clamped))(xt).numpy()          # [n][6], ambient
        return r, np.hstack([Ja[:, :3], Ja[:, 3:] @ sphere3_plus_jacobian(np.asarray(x[3:], dtype=np.float64))])[:, None, :]

    def plus(self, x, d):
        return np.concatenate([x[:3] + d[:3], sphere3_plus(x[3:], d[3:])])

    def finish(self, x):
        return x


class Homography:
    """x = H [3][3]; no manifold; the result is divided by H(2, 2)"""
    def __init__(self, corr, loss_type, loss_width):
        self.corr, self.loss, self.width = _t(corr).reshape(-1, 4), _LOSS[loss_type], loss_width

    def evaluate(self, x, jac):
        H = _t(x).reshape(3, 3)
        with np.errstate(all="ignore"):
            try:
                r = homography_residuals(H, self.corr).numpy()
            except RuntimeError:                                   # torch.linalg.inv refuses an exactly singular matrix
                return np.full((self.corr.shape[0], 4), np.nan), None
            if not jac or not np.all(np.isfinite(r)):
                return r, None
            J = jacrev(lambda z: homography_residuals(z, self.corr))(H).numpy().reshape(-1, 4, 9)
        return r, J

    def plus(self, x, d):
        return x + d.reshape(3, 3)

    def finish(self, x):
        with np.errstate(all="ignore"):
            return x / x[2, 2]


class Fundamental:
    """x = F [3][3]; 7 tangent dimensions; no loss"""
    def __init__(self, corr, loss_type=TRIVIAL, loss_width=1.0):
        assert loss_type == TRIVIAL
        self.corr, self.loss, self.width = _t(corr).reshape(-1, 4), "trivial", 1.0

    def evaluate(self, x, jac):
        F = _t(x).reshape(3, 3)
        with np.errstate(all="ignore"):
            r = sampson_residuals(F, self.corr).numpy().reshape(-1, 1)
            if not jac or not np.all(np.isfinite(r)):
                return r, None
            Ja = jacrev(lambda z: sampson_residuals(z, self.corr))(F).numpy().reshape(-1, 9)
            return r, (Ja @ fund_plus_jacobian(x))[:, None, :]

    def plus(self, x, d):
        return fund_plus(x, d)

    def finish(self, x):
        return x


def _corrected(P, x, jac):
    """cost, corrected residuals (flat), corrected Jacobian (flat rows): one loss per residual block, sqrt(rho') scaling"""
    r, J = P.evaluate(x, jac)
    s = (r * r).sum(1)
    rho, rho1 = ilm.loss(P.loss, P.width, s)
    sr = np.sqrt(rho1)
    cost = 0.5 * float(np.sum(rho)) if len(s) else 0.0
    rc = (r * sr[:, None]).reshape(-1)
    return cost, rc, (None if J is None else (J * sr[:, None, None]).reshape(len(rc), -1))


def initial_cost_longdouble(P, x):
    """sum of rho(|r|^2) / 2 in numpy.longdouble over the independent residuals"""
    r, _ = P.evaluate(x, False)
    s = (r.astype(np.longdouble) ** 2).sum(1)
    if P.loss == "huber":
        b = np.longdouble(P.width) ** 2
        rho = np.where(s > b, 2 * np.longdouble(P.width) * np.sqrt(s) - b, s)
    elif P.loss == "truncated":
        rho = np.minimum(s, np.longdouble(P.width) ** 2)
    else:
        rho = s
    return float(rho.sum() / 2) if len(s) else 0.0


def first_step(P, x0, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8):
    """One iteration (max_num_iterations = 1) from x0 at the initial trust-region radius.
    Returns (x after it -- x0 unless the step is accepted --, initial cost, accepted, iterations made: 0 for an empty
    problem, a non-finite initial cost and a gradient within its tolerance, else 1)."""
    x0 = np.array(x0, dtype=np.float64)
    if P.corr.shape[0] == 0:
        return P.finish(x0), 0.0, False, 0
    cost, r, J = _corrected(P, x0, True)
    if J is None or not np.isfinite(cost):
        return P.finish(x0), cost, False, 0
    scale = ilm.jacobi_scale(J)
    g = J.T @ r
    if np.abs(x0 - P.plus(x0, -g)).max() <= gradient_tolerance:
        return P.finish(x0), cost, False, 0
    ok, y, mcc = ilm.trial_step(J * scale, r, ilm.INITIAL_RADIUS)
    if not ok:
        return P.finish(x0), cost, False, 1
    cand = P.plus(x0, -y * scale)
    if not np.all(np.isfinite(cand)):
        return P.finish(x0), cost, False, 1
    cand_cost = _corrected(P, cand, False)[0]
    if not np.isfinite(cand_cost):
        cand_cost = np.finfo(np.float64).max
    change = cost - cand_cost
    if ilm.tolerance_stop(np.linalg.norm(x0 - cand), np.linalg.norm(x0), change, cost, parameter_tolerance, function_tolerance):
        return P.finish(x0), cost, False, 1
    if ilm.step_accepted(change / mcc):
        return P.finish(cand), cost, True, 1
    return P.finish(x0), cost, False, 1
