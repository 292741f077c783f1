"""Comparator for the Sim(3) alignment (tests/test_sim3_alignment.py, tests/test_sim3_alignment_gpu.py), written from the
reference's and Sophus' text; it shares nothing with pytheiasfm_amd/csrc/.

  * the maps in numpy, branch for branch: Sim3::exp (sim3.hpp:557-572) over RxSO3::expAndTheta (rxso3.hpp:600-619),
    SO3::expAndTheta (so3.hpp:584-620) and details::calcW (sim_details.hpp:10-49); Sim3::log (sim3.hpp:144-164) over
    RxSO3::logAndTheta, SO3::logAndTheta (so3.hpp:247-291) and calcWInv (sim_details.hpp:143-189); the conversions of
    align_point_clouds.cc:288-317 and transformation_wrapper.cc:125-132.  Tangent order: Sophus' [upsilon, omega, sigma].
  * the residuals of alignment_error.h:60-161; their Jacobians come from torch.func.jacfwd -- forward mode, as Ceres' Jets
    are -- over a torch transcription of exp (branches chosen on the values, as Jets choose them).
  * Ceres 2.2's trust-region loop restated from its rules, as tests/independent_lm.py does, with the options
    align_point_clouds.cc:258-266 leave: function tolerance 1e-6, gradient tolerance 1e-10, parameter tolerance 1e-8, initial
    radius 1e4, max radius 1e16, Jacobi scaling; the 7 x 7 normal equations by numpy's Cholesky.  `sum_dtype` is the type the
    sums over the points are taken in (float64 or longdouble): the spread between the two is the yardstick the device's
    tolerance is stated in."""
import numpy as np
import torch
from torch.func import jacfwd

EPS = 1e-10
EPS_PLUS = EPS * (1.0 + EPS)
POINT_TO_POINT, ROBUST_POINT_TO_POINT, POINT_TO_PLANE = 0, 1, 2
TERM_NO_POINTS, TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS, TERM_FAILURE, TERM_MIN_RADIUS = range(7)
CONVERGED = (TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_MIN_RADIUS)


def hat(o):
    return np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])


def so3_exp_quat(omega):
    """SO3::expAndTheta -> (w, v [3], theta)"""
    theta_sq = float(omega @ omega)
    if theta_sq < EPS * EPS:
        theta = 0.0
        po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * po4
    else:
        theta = np.sqrt(theta_sq)
        half = 0.5 * theta
        imag = np.sin(half) / theta
        real = np.cos(half)
    return real, imag * omega, theta


def rxso3_matrix(w, v):
    x, y, z = v
    return np.array([[x * x - y * y - z * z + w * w, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, -x * x + y * y - z * z + w * w, -2 * x * w + 2 * y * z],
                     [2 * x * z - 2 * y * w, 2 * x * w + 2 * y * z, -x * x - y * y + z * z + w * w]])


def calc_w(omega, theta, sigma):
    Om = hat(omega)
    Om2 = Om @ Om
    scale = np.exp(sigma)
    if abs(sigma) < EPS:
        C = 1.0
        if abs(theta) < EPS:
            A, B = 0.5, 1.0 / 6.0
        else:
            A = (1.0 - np.cos(theta)) / (theta * theta)
            B = (theta - np.sin(theta)) / (theta * theta * theta)
    else:
        C = (scale - 1.0) / sigma
        if abs(theta) < EPS:
            s2 = sigma * sigma
            A = ((sigma - 1.0) * scale + 1.0) / s2
            B = (scale * 0.5 * s2 + scale - 1.0 - sigma * scale) / (s2 * sigma)
        else:
            a, b = scale * np.sin(theta), scale * np.cos(theta)
            c = theta * theta + sigma * sigma
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) / (theta * theta)
    return A * Om + B * Om2 + C * np.eye(3)


def branch(a):
    """(small sigma, small theta) as calcW decides them"""
    a = np.asarray(a, dtype=np.float64)
    return bool(abs(a[6]) < EPS), bool(float(a[3:6] @ a[3:6]) < EPS * EPS)


def sim3_exp(a):
    """-> sR [3][3] (rxso3().matrix()), t [3]"""
    a = np.asarray(a, dtype=np.float64)
    ups, omega, sigma = a[:3], a[3:6], a[6]
    scale = min(max(np.exp(sigma), EPS_PLUS), 1.0 / EPS_PLUS)
    w, v, theta = so3_exp_quat(omega)
    ss = np.sqrt(scale)
    return rxso3_matrix(w * ss, v * ss), calc_w(omega, theta, sigma) @ ups


def quat_from_rot(m):
    """Eigen::Quaternion(Matrix3) -> (w, v)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    v = np.zeros(3)
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        v[:] = [(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        v[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        v[j] = (m[j, i] + m[i, j]) * t
        v[k] = (m[k, i] + m[i, k]) * t
    return w, v


def sim3_log(scale_in, R, t):
    """Sim3d(RxSO3d(scale, R), t).log()"""
    R = np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    w, v = quat_from_rot(R)
    ss = np.sqrt(scale_in)
    w, v = w * ss, v * ss
    scale = float(v @ v) + w * w
    sigma = np.log(scale)
    n_q = np.sqrt(scale)
    w, v = w / n_q, v / n_q
    sq_n = float(v @ v)
    if sq_n < EPS * EPS:
        f = 2.0 / w - (2.0 / 3.0) * sq_n / (w * w * w)
        theta = 2.0 * sq_n / w
    else:
        n = np.sqrt(sq_n)
        if abs(w) < EPS:
            f = np.pi / n if w > 0 else -np.pi / n
        else:
            f = 2.0 * np.arctan(n / w) / n
        theta = f * n
    omega = f * v
    Om = hat(omega)
    Om2 = Om @ Om
    th2 = theta * theta
    s, c = np.sin(theta), np.cos(theta)
    if abs(sigma * sigma) < EPS:
        cc = 1.0 - 0.5 * sigma
        ca = -0.5
        cb = 1.0 / 12.0 if abs(th2) < EPS else (theta * s + 2.0 * c - 2.0) / (2.0 * th2 * (c - 1.0))
    else:
        cc = sigma / (scale - 1.0)
        if abs(th2) < EPS:
            ca = (-sigma * scale + scale - 1.0) / ((scale - 1.0) * (scale - 1.0))
            cb = (scale * scale * sigma - 2.0 * scale * scale + scale * sigma + 2.0 * scale) / \
                 (2.0 * scale ** 3 - 6.0 * scale * scale + 6.0 * scale - 2.0)
        else:
            ss_, sc_ = scale * s, scale * c
            ca = (theta * sc_ - theta - sigma * ss_) / (theta * (scale * scale - 2.0 * sc_ + 1.0))
            cb = -scale * (theta * ss_ - theta * s + sigma * sc_ - scale * sigma + sigma * c - sigma) / \
                 (th2 * (scale ** 3 - 2.0 * scale * sc_ - scale * scale + 2.0 * sc_ + scale - 1.0))
    Winv = ca * Om + cb * Om2 + cc * np.eye(3)
    return np.concatenate([Winv @ t, omega, [sigma]])


def sim3_from_rts(R, t, scale):
    return sim3_log(scale, R, t)


def sim3_to_rts(a):
    a = np.asarray(a, dtype=np.float64)
    _, t = sim3_exp(a)
    scale = min(max(np.exp(a[6]), EPS_PLUS), 1.0 / EPS_PLUS)
    w, v, _ = so3_exp_quat(a[3:6])
    ss = np.sqrt(scale)
    w, v = w * ss, v * ss
    sq = float(v @ v) + w * w
    n = np.sqrt(sq)
    w, v = w / n, v / n
    x, y, z = v
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, t, sq


def sim3_to_matrix4(a):
    sR, t = sim3_exp(a)
    M = np.eye(4)
    M[:3, :3] = sR
    M[:3, 3] = t
    return M


# ---- torch: exp with the branches of the VALUE (what a Jet's comparison operators look at)
_LEVI = torch.zeros((3, 3, 3), dtype=torch.float64)            # hat(o)[i][j] = sum_k _LEVI[i][j][k] o[k]
for _i, _j, _k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
    _LEVI[_i, _j, _k] = -1.0
    _LEVI[_j, _i, _k] = 1.0


def _t_hat(o):
    return _LEVI @ o


def torch_exp(a, small_sigma, small_rot, clamp_value=None):
    """Sim3::exp on a torch vector with the branches given (python bools; clamp_value: the constant the clamp of exp(sigma)
    returned, when it acted) -> sR [3][3], t [3]"""
    ups, omega, sigma = a[:3], a[3:6], a[6]
    one = torch.ones((), dtype=a.dtype)
    scale = torch.exp(sigma)
    scale_c = scale if clamp_value is None else one * clamp_value
    theta_sq = (omega * omega).sum()
    if small_rot:
        theta = torch.zeros((), dtype=a.dtype)
        po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * po4
    else:
        theta = torch.sqrt(theta_sq)
        half = 0.5 * theta
        imag = torch.sin(half) / theta
        real = torch.cos(half)
    ss = torch.sqrt(scale_c)
    w = real * ss
    v = (imag * ss) * omega
    # rxso3().matrix() of the quaternion (w, v): (w^2 - v.v) I + 2 v v' + 2 w hat(v)
    sR = (w * w - (v * v).sum()) * torch.eye(3, dtype=a.dtype) + 2.0 * torch.outer(v, v) + (2.0 * w) * _t_hat(v)
    Om = _t_hat(omega)
    Om2 = Om @ Om
    if small_sigma:
        C = one
        if small_rot:
            A, B = 0.5 * one, one / 6.0
        else:
            A = (1.0 - torch.cos(theta)) / (theta * theta)
            B = (theta - torch.sin(theta)) / (theta * theta * theta)
    else:
        C = (scale - 1.0) / sigma
        if small_rot:
            s2 = sigma * sigma
            A = ((sigma - 1.0) * scale + 1.0) / s2
            B = (scale * 0.5 * s2 + scale - 1.0 - sigma * scale) / (s2 * sigma)
        else:
            a_, b_ = scale * torch.sin(theta), scale * torch.cos(theta)
            c_ = theta * theta + sigma * sigma
            A = (a_ * sigma + (1.0 - b_) * theta) / (theta * c_)
            B = (C - ((b_ - 1.0) * sigma + a_ * theta) / c_) / (theta * theta)
    W = A * Om + B * Om2 + C * torch.eye(3, dtype=a.dtype)
    return sR, W @ ups


def exp_jacobian(a):
    """d(sR [9] row-major | t [3]) / da [12][7] by forward-mode autodiff of the branch `a` takes"""
    a = np.asarray(a, dtype=np.float64)
    ssig, srot = branch(a)
    sc = np.exp(a[6])
    clamp_value = None if EPS_PLUS <= sc <= 1.0 / EPS_PLUS else min(max(sc, EPS_PLUS), 1.0 / EPS_PLUS)

    def f(v):
        sR, t = torch_exp(v, ssig, srot, clamp_value)
        return torch.cat([sR.reshape(-1), t])
    return jacfwd(f)(torch.tensor(a, dtype=torch.float64)).numpy()


def residuals(a, prob, jac):
    """r [n][m], J [n][m][7] (or None) of the problem's residual blocks at a, before the loss.  The residuals are linear
    in (sR, t), so their Jacobians are jacfwd's derivative of exp carried through that linear map."""
    sR, t = sim3_exp(a)
    d = prob.y - (prob.x @ sR.T + t)
    plane = prob.kind == POINT_TO_PLANE
    r = (prob.w * (prob.nn * d).sum(1))[:, None] if plane else prob.w[:, None] * d
    if not jac:
        return r, None
    E = exp_jacobian(a)                                                   # [12][7]: sR row-major, then t
    M = np.einsum("rck,nc->nrk", E[:9].reshape(3, 3, 7), prob.x) + E[9:][None]   # d(sR x + t) / da [n][3][7]
    J = -prob.w[:, None, None] * (np.einsum("nr,nrk->nk", prob.nn, M)[:, None, :] if plane else M)
    return r, J


class Problem:
    """One alignment problem.  alignment_type POINT_TO_PLANE without normals is point-to-point (:228-238)."""

    def __init__(self, source, target, alignment_type=POINT_TO_POINT, weights=None, normals=None, point_weight=1.0,
                 huber_threshold=0.1):
        self.x = np.asarray(source, dtype=np.float64).reshape(-1, 3)
        self.y = np.asarray(target, dtype=np.float64).reshape(-1, 3)
        n = self.x.shape[0]
        self.w = np.full(n, float(point_weight)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        self.kind = alignment_type
        if alignment_type == POINT_TO_PLANE and normals is None:
            self.kind = POINT_TO_POINT
        nn = np.ones((n, 3))
        if self.kind == POINT_TO_PLANE:
            nn = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
            nn = nn / np.sqrt((nn * nn).sum(1))[:, None]      # the functor's constructor: target_normal.normalized()
        self.huber = float(huber_threshold)
        self.nn = nn

    def evaluate(self, a, jac, sum_dtype=np.float64):
        """cost, J'r [7], J'J [7][7] with the loss's corrector applied; the sums over the points in sum_dtype"""
        r, J = residuals(a, self, jac)
        s = (r * r).sum(1)
        if self.kind == ROBUST_POINT_TO_POINT:                 # ceres::HuberLoss; rho'' <= 0: scale by sqrt(rho')
            b = self.huber * self.huber
            out = s > b
            root = np.sqrt(np.where(out, s, 1.0))
            rho = np.where(out, 2.0 * self.huber * root - b, s)
            sq = np.sqrt(np.where(out, np.maximum(np.finfo(np.float64).tiny, self.huber / root), 1.0))
        else:
            rho, sq = s, np.ones_like(s)
        cost = 0.5 * float(rho.astype(sum_dtype).sum(dtype=sum_dtype))
        if not jac:
            return cost, None, None
        rc = r * sq[:, None]
        Jc = J * sq[:, None, None]
        g = np.einsum("nmk,nm->nk", Jc, rc).astype(sum_dtype).sum(0, dtype=sum_dtype)
        H = np.einsum("nma,nmb->nab", Jc, Jc).astype(sum_dtype).sum(0, dtype=sum_dtype)
        return cost, g.astype(np.float64), H.astype(np.float64)

    def alignment_error(self, a):
        sR, t = sim3_exp(a)
        return float(np.sqrt((((self.x @ sR.T + t) - self.y) ** 2).sum(1)).mean())


class Result:
    pass


def solve(prob, start, max_iterations=100, sum_dtype=np.float64, function_tolerance=1e-6, gradient_tolerance=1e-10,
          parameter_tolerance=1e-8, max_radius=1e16):
    """Ceres' loop.  Returns a Result: params, termination, success, num_iterations (= summary.iterations.size()), counts,
    initial_cost, final_cost, alignment_error, trace rows (cost, gradient max norm, step norm, radius, accepted) and
    last_rel_change, the last accepted step's |cost change| / cost."""
    res = Result()
    x = np.array(start, dtype=np.float64)
    x0 = x.copy()
    res.trace = []
    res.successful = res.unsuccessful = res.invalid = 0
    res.last_rel_change = np.inf
    if prob.x.shape[0] == 0:
        res.params, res.termination, res.success, res.num_iterations = x, TERM_NO_POINTS, False, 0
        res.initial_cost = res.final_cost = res.alignment_error = 0.0
        return res
    cost, g, H = prob.evaluate(x, True, sum_dtype)
    res.initial_cost = cost
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    gmax = float(np.abs(g).max())
    x_norm = float(np.linalg.norm(x))
    radius, decrease, invalid_row, successful = 1e4, 2.0, 0, True
    res.trace.append((cost, gmax, 0.0, radius, 1))
    pushed = 1
    while True:
        if pushed - 1 >= max_iterations:
            term = TERM_MAX_ITERATIONS
            break
        if successful and gmax <= gradient_tolerance:
            term = TERM_GRADIENT
            break
        if radius <= 1e-32:
            term = TERM_MIN_RADIUS
            break
        gs = g * scale
        Hs = H * scale[:, None] * scale[None, :]
        D = np.clip(np.diag(Hs), 1e-6, 1e32) / radius
        try:
            L = np.linalg.cholesky(Hs + np.diag(D))
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            ok = False
        model = 0.0
        if ok:
            model = float(y @ gs - 0.5 * (y @ (Hs @ y)))
            ok = bool(np.isfinite(model) and model > 0.0)
        if not ok:
            res.invalid += 1
            invalid_row += 1
            if invalid_row >= 5:
                term = TERM_FAILURE
                x = x0.copy()
                break
            radius /= decrease
            decrease *= 2.0
            successful = False
            res.trace.append((cost, gmax, 0.0, radius, 0))
            pushed += 1
            continue
        invalid_row = 0
        delta = -(y * scale)
        xc = x + delta
        step_norm = float(np.linalg.norm(delta))
        cand, gc, Hc = prob.evaluate(xc, True, sum_dtype)
        if not np.isfinite(cand):
            cand = np.finfo(np.float64).max
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            res.trace.append((cand, gmax, step_norm, radius, 0))
            term = TERM_PARAMETER
            break
        if abs(cost - cand) <= function_tolerance * cost:
            res.trace.append((cand, gmax, step_norm, radius, 0))
            term = TERM_FUNCTION
            break
        rho = (cost - cand) / model
        if rho > 1e-3:
            res.last_rel_change = abs(cost - cand) / cost
            x, g, H = xc, gc, Hc
            x_norm = float(np.linalg.norm(x))
            cost = cand
            gmax = float(np.abs(g).max())
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, successful = 2.0, True
            res.successful += 1
            res.trace.append((cost, gmax, step_norm, radius, 1))
        else:
            radius /= decrease
            decrease *= 2.0
            successful = False
            res.unsuccessful += 1
            res.trace.append((cand, gmax, step_norm, radius, 0))
        pushed += 1
    res.params, res.termination, res.success, res.num_iterations = x, term, term in CONVERGED, pushed
    res.final_cost = cost
    res.alignment_error = prob.alignment_error(x)
    return res


# ---- the reference's scenes (align_point_clouds_test.cc)
def rotation_from_axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = hat(axis)
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def synthetic_cloud(n, noise, rng=None):
    """GenerateSyntheticPointCloud (:204-220): the curve x = 10 (i / n - 1 / 2), y = 5 sin(x / 2), z = 2 cos(0.3 x), each
    coordinate with N(0, noise) added (numpy's generator in place of the reference's)"""
    x = 10.0 * (np.arange(n) / n - 0.5)
    p = np.stack([x, 5.0 * np.sin(x * 0.5), 2.0 * np.cos(x * 0.3)], axis=1)
    if noise > 0.0:
        p = p + rng.normal(0.0, noise, size=(n, 3))
    return p


def transform_cloud(points, a):
    """TransformPointCloud (:223-234)"""
    sR, t = sim3_exp(a)
    return np.asarray(points) @ sR.T + t


def umeyama(source, target):
    """AlignPointCloudsUmeyama (align_point_clouds.cc:45-150, unit weights) in numpy -> R, t, scale"""
    x, y = np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64)
    xc, yc = x.mean(0), y.mean(0)
    dx, dy = x - xc, y - yc
    sigma = (dx * dx).sum() / len(x)
    U, S, Vt = np.linalg.svd(dy.T @ dx / len(x))
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    scale = float((S * d).sum() / sigma)
    return R, yc - scale * (R @ xc), scale


def create_sim3(translation, rotation_axis_angle, scale):
    """CreateSim3Transformation (:237-253)"""
    w = np.asarray(rotation_axis_angle, dtype=np.float64)
    angle = float(np.linalg.norm(w))
    R = rotation_from_axis_angle(w / angle, angle) if angle > 1e-8 else np.eye(3)
    return sim3_log(scale, R, np.asarray(translation, dtype=np.float64))
