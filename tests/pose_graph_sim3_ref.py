"""Comparator for the Sim(3) pose graph (tests/test_pose_graph_sim3.py, tests/test_pose_graph_sim3_gpu.py), written from the
reference's headers over tests/sim3_ref.py; it shares nothing with pytheiasfm_amd/csrc/.

  * the term Sim3ReconAlignErrorTerm (pose_graph_sim3_error.h:46-103) in numpy, with its 7 x 7 matrices multiplied out as the
    reference writes them: r = log(Sji exp(x_i) exp(x_j)^-1); Jr0 from the UNWEIGHTED r; J_i = sqrt_information (I + Jr0 / 2 +
    Jr0^2 / 12) Adj(exp(x_j)), J_j = -J_i; residual = sqrt_information r.  Group elements are (scale, R, t) from
    sim3_ref.sim3_to_rts, the logarithm is sim3_ref.sim3_log.
  * Sim3Manifold::Plus (align_reconstructions_pose_graph_optim.cc:39-56): log(exp(x) exp(d')), d'[6] = max(d[6], -20).
  * the same term in mpmath (50 digits), formula for formula and branch for branch: what the term tests measure the numpy
    term's own error against.
  * Ceres 2.2's trust-region loop in the conventions of sim3_ref.solve, over a graph with held nodes, at
    ceres::Solver::Options' defaults; the dense normal equations by numpy's Cholesky.  `sum_dtype` is the type the sums over
    the edges are taken in (float64 or longdouble).  Counts are the device's: `iterations` = passes of the loop."""
import mpmath as mp
import numpy as np

from tests import sim3_ref as ref

TERM_NONE, TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS, TERM_FAILURE, TERM_MIN_RADIUS = range(7)
I7 = np.eye(7)


# ---- the group on (scale, R, t): x -> scale R x + t
def group(a):
    R, t, s = ref.sim3_to_rts(a)
    return s, R, t


def mul(A, B):
    return A[0] * B[0], A[1] @ B[1], A[0] * (A[1] @ B[2]) + A[2]


def inv(A):
    s, R, t = A
    return 1.0 / s, R.T, -((R.T @ t) / s)


def log(A):
    """None where Sophus' log would abort (a scale outside [1e-10, 1e10))"""
    if not (ref.EPS <= A[0] < 1.0 / ref.EPS):
        return None
    return ref.sim3_log(A[0], A[1], A[2])


def adjoint(A):
    """Sophus' Sim3::Adj() (sim3.hpp): [sR hat(t) R -t; 0 R 0; 0 0 1]"""
    s, R, t = A
    M = np.zeros((7, 7))
    M[:3, :3] = s * R
    M[:3, 3:6] = ref.hat(t) @ R
    M[:3, 6] = -t
    M[3:6, 3:6] = R
    M[6, 6] = 1.0
    return M


def residual(xi, xj, z):
    """the unweighted r = log(Sji exp(x_i) exp(x_j)^-1), z = log(Sji)"""
    return log(mul(group(z), mul(group(xi), inv(group(xj)))))


def jr0(r):
    J = np.zeros((7, 7))
    J[:3, :3] = ref.hat(r[3:6]) + r[6] * np.eye(3)     # RxSO3::hat(residuals.tail(4))
    J[:3, 3:6] = ref.hat(r[:3])
    J[:3, 6] = -r[:3]
    J[3:6, 3:6] = ref.hat(r[3:6])
    return J


def series(r):
    J = jr0(r)
    return I7 + 0.5 * J + (1.0 / 12.0) * (J @ J)


def term(xi, xj, z, W=None, jac=True):
    """-> weighted residual [7], J_i [7][7] (None without jac)"""
    W = I7 if W is None else W
    r = residual(xi, xj, z)
    if r is None:
        return np.full(7, np.nan), (np.full((7, 7), np.nan) if jac else None)
    if not jac:
        return W @ r, None
    return W @ r, (W @ series(r)) @ adjoint(group(xj))


def plus(x, d):
    """Sim3Manifold::Plus; None where the logarithm is not defined"""
    d = np.array(d, dtype=np.float64)
    d[6] = max(d[6], -20.0)
    return log(mul(group(x), group(d)))


def relative(xi, xj):
    """log(exp(x_j) exp(x_i)^-1): the measurement that makes the residual of edge (i, j) zero"""
    return log(mul(group(xj), inv(group(xi))))


# ---- the same term in mpmath
DPS = 50


def _m_hat(o):
    return mp.matrix([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])


def _m_group(a):
    a = [mp.mpf(float(v)) for v in a]
    ups, om, sig = mp.matrix(a[:3]), mp.matrix(a[3:6]), a[6]
    th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    eps = mp.mpf(ref.EPS)
    if th2 < eps * eps:
        theta = mp.mpf(0)
        imag = mp.mpf(1) / 2 - th2 / 48 + th2 * th2 / 3840
        real = 1 - th2 / 8 + th2 * th2 / 384
    else:
        theta = mp.sqrt(th2)
        imag = mp.sin(theta / 2) / theta
        real = mp.cos(theta / 2)
    scale_raw = mp.exp(sig)
    eps_plus = eps * (1 + eps)
    scale = min(max(scale_raw, eps_plus), 1 / eps_plus)
    ss = mp.sqrt(scale)
    w, v = real * ss, imag * ss * om
    sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + w * w
    n = mp.sqrt(sq)
    w, x, y, z = w / n, v[0] / n, v[1] / n, v[2] / n
    R = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Om = _m_hat(om)
    Om2 = Om * Om
    if abs(sig) < eps:
        C = mp.mpf(1)
        if abs(theta) < eps:
            A, B = mp.mpf(1) / 2, mp.mpf(1) / 6
        else:
            A = (1 - mp.cos(theta)) / (theta * theta)
            B = (theta - mp.sin(theta)) / (theta * theta * theta)
    else:
        C = (scale_raw - 1) / sig
        if abs(theta) < eps:
            s2 = sig * sig
            A = ((sig - 1) * scale_raw + 1) / s2
            B = (scale_raw * s2 / 2 + scale_raw - 1 - sig * scale_raw) / (s2 * sig)
        else:
            a_, b_ = scale_raw * mp.sin(theta), scale_raw * mp.cos(theta)
            c_ = theta * theta + sig * sig
            A = (a_ * sig + (1 - b_) * theta) / (theta * c_)
            B = (C - ((b_ - 1) * sig + a_ * theta) / c_) / (theta * theta)
    Wm = A * Om + B * Om2 + C * mp.eye(3)
    return sq, R, Wm * ups


def _m_mul(A, B):
    return A[0] * B[0], A[1] * B[1], A[0] * (A[1] * B[2]) + A[2]


def _m_inv(A):
    s, R, t = A
    return 1 / s, R.T, -((R.T * t) / s)


def _m_log(A):
    s_in, m, t = A
    eps = mp.mpf(ref.EPS)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    v = [mp.mpf(0)] * 3
    if tr > 0:
        tr = mp.sqrt(tr + 1)
        w = tr / 2
        tr = 1 / (2 * tr)
        v = [(m[2, 1] - m[1, 2]) * tr, (m[0, 2] - m[2, 0]) * tr, (m[1, 0] - m[0, 1]) * tr]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tr = mp.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        v[i] = tr / 2
        tr = 1 / (2 * tr)
        w = (m[k, j] - m[j, k]) * tr
        v[j] = (m[j, i] + m[i, j]) * tr
        v[k] = (m[k, i] + m[i, k]) * tr
    ss = mp.sqrt(s_in)
    w, v = w * ss, [c * ss for c in v]
    scale = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + w * w
    sigma = mp.log(scale)
    nq = mp.sqrt(scale)
    w, v = w / nq, [c / nq for c in v]
    sq_n = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if sq_n < eps * eps:
        f = 2 / w - (mp.mpf(2) / 3) * sq_n / (w * w * w)
        theta = 2 * sq_n / w
    else:
        n = mp.sqrt(sq_n)
        if abs(w) < eps:
            f = mp.pi / n if w > 0 else -mp.pi / n
        else:
            f = 2 * mp.atan(n / w) / n
        theta = f * n
    omega = mp.matrix([f * c for c in v])
    Om = _m_hat(omega)
    Om2 = Om * Om
    th2 = theta * theta
    s, c = mp.sin(theta), mp.cos(theta)
    if abs(sigma * sigma) < eps:
        cc = 1 - sigma / 2
        ca = -mp.mpf(1) / 2
        cb = mp.mpf(1) / 12 if abs(th2) < eps else (theta * s + 2 * c - 2) / (2 * th2 * (c - 1))
    else:
        cc = sigma / (scale - 1)
        if abs(th2) < eps:
            ca = (-sigma * scale + scale - 1) / ((scale - 1) * (scale - 1))
            cb = (scale * scale * sigma - 2 * scale * scale + scale * sigma + 2 * scale) / \
                 (2 * scale ** 3 - 6 * scale * scale + 6 * scale - 2)
        else:
            ss_, sc_ = scale * s, scale * c
            ca = (theta * sc_ - theta - sigma * ss_) / (theta * (scale * scale - 2 * sc_ + 1))
            cb = -scale * (theta * ss_ - theta * s + sigma * sc_ - scale * sigma + sigma * c - sigma) / \
                 (th2 * (scale ** 3 - 2 * scale * sc_ - scale * scale + 2 * sc_ + scale - 1))
    u = (ca * Om + cb * Om2 + cc * mp.eye(3)) * t
    return [u[0], u[1], u[2], omega[0], omega[1], omega[2], sigma]


def term_mp(xi, xj, z, W=None):
    """the term of term() evaluated in mpmath (DPS digits) on the same float64 inputs -> residual [7], J_i [7][7] as
    float64-rounded numpy arrays"""
    with mp.workdps(DPS):
        return _term_mp(xi, xj, z, W)


def _term_mp(xi, xj, z, W):
    Wm =mp.eye(7) if W is None else mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(W)])
    Sj = _m_group(xj)
    r = _m_log(_m_mul(_m_group(z), _m_mul(_m_group(xi), _m_inv(Sj))))
    J = mp.zeros(7, 7)
    O, U = _m_hat(r[3:6]), _m_hat(r[:3])
    for a in range(3):
        for b in range(3):
            J[a, b] = O[a, b] + (r[6] if a == b else 0)
            J[a, 3 + b] = U[a, b]
            J[3 + a, 3 + b] = O[a, b]
        J[a, 6] = -r[a]
    M = mp.eye(7) + J / 2 + (J * J) / 12
    s, R, t = Sj
    Adj = mp.zeros(7, 7)
    TR = _m_hat(t) * R
    for a in range(3):
        for b in range(3):
            Adj[a, b] = s * R[a, b]
            Adj[a, 3 + b] = TR[a, b]
            Adj[3 + a, 3 + b] = R[a, b]
        Adj[a, 6] = -t[a]
    Adj[6, 6] = 1
    Ji = (Wm * M) * Adj
    res = Wm * mp.matrix(r)
    return (np.array([float(res[k]) for k in range(7)]),
            np.array([[float(Ji[a, b]) for b in range(7)] for a in range(7)]))


# ---- the problem and Ceres' loop
class Graph:
    """nodes [n][7], edges [E][2] = (i, j), measurements [E][7], sqrt_information [E][7][7] or None, fixed [n] or None"""

    def __init__(self, nodes, edges, measurements, sqrt_information=None, fixed=None):
        self.x0 = np.array(nodes, dtype=np.float64).reshape(-1, 7)
        self.edges = np.array(edges, dtype=np.int64).reshape(-1, 2)
        self.z = np.array(measurements, dtype=np.float64).reshape(-1, 7)
        E, n = len(self.edges), len(self.x0)
        self.W = None if sqrt_information is None else np.array(sqrt_information, dtype=np.float64).reshape(E, 7, 7)
        held = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool).copy()
        touched = np.zeros(n, dtype=bool)
        touched[self.edges.reshape(-1)] = True
        self.free = np.flatnonzero(touched & ~held)
        self.idx = np.full(n, -1)
        self.idx[self.free] = np.arange(len(self.free))
        # an edge between two held nodes is not in the problem
        self.active = [e for e, (i, j) in enumerate(self.edges) if self.idx[i] >= 0 or self.idx[j] >= 0]

    def weight(self, e):
        return None if self.W is None else self.W[e]

    def cost(self, x, sum_dtype=np.float64):
        s = sum_dtype(0.0)
        for e in self.active:
            i, j = self.edges[e]
            r, _ = term(x[i], x[j], self.z[e], self.weight(e), jac=False)
            s += sum_dtype(float(r @ r))
        return 0.5 * float(s)

    def linearise(self, x, sum_dtype=np.float64):
        """cost, the edges' records [(e, r, J_i)]"""
        recs, s = [], sum_dtype(0.0)
        for e in self.active:
            i, j = self.edges[e]
            r, J = term(x[i], x[j], self.z[e], self.weight(e))
            recs.append((e, r, J))
            s += sum_dtype(float(r @ r))
        return 0.5 * float(s), recs

    def normal_equations(self, recs, scale, sum_dtype=np.float64):
        """unscaled gradient J'r [7m] and the scaled Js'Js [7m][7m], sums over the edges in sum_dtype"""
        m = len(self.free)
        g = np.zeros(7 * m, dtype=sum_dtype)
        H = np.zeros((7 * m, 7 * m), dtype=sum_dtype)
        for e, r, J in recs:
            i, j = self.edges[e]
            ends = [(self.idx[i], 1.0), (self.idx[j], -1.0)]
            for a, sa in ends:
                if a < 0:
                    continue
                g[7 * a:7 * a + 7] += (sa * (J.T @ r)).astype(sum_dtype)
                Ja = sa * J * scale[7 * a:7 * a + 7][None, :]
                for b, sb in ends:
                    if b < 0:
                        continue
                    Jb = sb * J * scale[7 * b:7 * b + 7][None, :]
                    H[7 * a:7 * a + 7, 7 * b:7 * b + 7] += (Ja.T @ Jb).astype(sum_dtype)
        return g.astype(np.float64), H.astype(np.float64)

    def column_scale(self, recs):
        m = len(self.free)
        sq = np.zeros(7 * m)
        for e, r, J in recs:
            for a in (self.idx[self.edges[e][0]], self.idx[self.edges[e][1]]):
                if a >= 0:
                    sq[7 * a:7 * a + 7] += (J * J).sum(0)
        return 1.0 / (1.0 + np.sqrt(sq))


class Result:
    pass


def solve(graph, max_iterations=50, sum_dtype=np.float64, function_tolerance=1e-6, gradient_tolerance=1e-10,
          parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16):
    """Ceres' loop.  Returns a Result: nodes, termination, iterations, successful, unsuccessful, invalid, initial_cost,
    final_cost, trace rows (cost, gradient max norm, step norm, radius, accepted) and last_rel_change, the last accepted
    step's |cost change| / cost."""
    res = Result()
    x = graph.x0.copy()
    free, m = graph.free, len(graph.free)
    res.trace = []
    res.iterations = res.successful = res.unsuccessful = res.invalid = 0
    res.last_rel_change = np.inf
    res.nodes = x
    res.initial_cost = res.final_cost = 0.0
    if m == 0:
        res.termination = TERM_NONE
        return res
    cost, recs = graph.linearise(x, sum_dtype)
    scale = graph.column_scale(recs)
    g, H = graph.normal_equations(recs, scale, sum_dtype)
    res.initial_cost = cost
    gmax = float(np.abs(g).max())
    x_norm = float(np.linalg.norm(x[free]))
    radius, decrease, invalid_row, successful = initial_radius, 2.0, 0, True
    res.trace.append([cost, gmax, 0.0, radius, 1])
    term_code = TERM_GRADIENT if gmax <= gradient_tolerance else None
    while term_code is None:
        if res.iterations >= max_iterations:
            term_code = TERM_MAX_ITERATIONS
            break
        if successful and gmax <= gradient_tolerance:
            term_code = TERM_GRADIENT
            break
        if radius <= 1e-32:
            term_code = TERM_MIN_RADIUS
            break
        res.iterations += 1
        gs = g * scale
        D = np.clip(np.diag(H), 1e-6, 1e32) / radius
        xc, ok = x.copy(), True
        try:
            L = np.linalg.cholesky(H + np.diag(D))
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            ok = False
        model = 0.0
        if ok:
            delta = -(y * scale)
            for a, v in enumerate(free):
                p = plus(x[v], delta[7 * a:7 * a + 7])
                if p is None:
                    ok = False
                    break
                xc[v] = p
        if ok:
            model = float(y @ gs - 0.5 * (y @ (H @ y)))
            ok = bool(np.isfinite(model) and model > 0.0)
        if not ok:
            res.invalid += 1
            invalid_row += 1
            if invalid_row >= 5:
                term_code = TERM_FAILURE
                x = graph.x0.copy()
                break
            radius /= decrease
            decrease *= 2.0
            successful = False
            res.trace.append([cost, gmax, 0.0, radius, 0])
            continue
        invalid_row = 0
        step_norm = float(np.linalg.norm(xc[free] - x[free]))
        cand, recs_c = graph.linearise(xc, sum_dtype)        # every candidate with its Jacobian, as sim3_ref.solve
        if not np.isfinite(cand):
            cand = np.finfo(np.float64).max
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            res.trace.append([cand, gmax, step_norm, radius, 0])
            term_code = TERM_PARAMETER
            break
        if abs(cost - cand) <= function_tolerance * cost:
            res.trace.append([cand, gmax, step_norm, radius, 0])
            term_code = TERM_FUNCTION
            break
        rho = (cost - cand) / model
        if rho > 1e-3:
            res.last_rel_change = abs(cost - cand) / cost
            x = xc
            x_norm = float(np.linalg.norm(x[free]))
            cost, recs = cand, recs_c
            g, H = graph.normal_equations(recs, scale, sum_dtype)
            gmax = float(np.abs(g).max())
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, successful = 2.0, True
            res.successful += 1
            res.trace.append([cost, gmax, step_norm, radius, 1])
        else:
            radius /= decrease
            decrease *= 2.0
            successful = False
            res.unsuccessful += 1
            res.trace.append([cand, gmax, step_norm, radius, 0])
    res.nodes, res.termination, res.final_cost = x, term_code, cost
    res.final_radius, res.final_gradient_max_norm = radius, gmax
    res.trace = np.array(res.trace)
    return res


# ---- scenes
def ring_scene(n, seed, with_information=False, chords=True, noise=1e-3, drift=0.02):
    """n cameras on a ring looking inwards (node 0 held), edges (k, k + 1) around the ring and a chord (k, k + 3) from every
    fourth node; measurements = the ground truth's relative Sim(3) with `noise` added in the tangent; the start = the ground
    truth moved by `drift` (nodes 1 ..).  -> Graph, ground truth [n][7]"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, 7))
    for k in range(n):
        ang = 2.0 * np.pi * k / max(n, 3)
        R = ref.rotation_from_axis_angle([0.1, 1.0, 0.05], ang + 0.3)
        C = np.array([4.0 * np.cos(ang), 0.2 * np.sin(3.0 * ang), 4.0 * np.sin(ang)])
        gt[k] = ref.sim3_log(float(np.exp(0.1 * np.sin(ang))), R, -R @ C)
    edges = [(k, (k + 1) % n) for k in range(n if n > 2 else 1)]
    if chords:
        edges += [(k, (k + 3) % n) for k in range(0, n, 4) if n > 4]
    edges = np.array(edges)
    z = np.array([relative(gt[i], gt[j]) for i, j in edges]) + noise * rng.standard_normal((len(edges), 7))
    start = gt.copy()
    start[1:] += drift * rng.standard_normal((n - 1, 7))
    W = None
    if with_information:
        W = np.tile(np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5]), (len(edges), 1, 1)) + \
            0.05 * rng.standard_normal((len(edges), 7, 7))
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    return Graph(start, edges, z, W, fixed), gt
