"""Edge scenes of the three wavefront LM solvers of csrc/twoview_lm.hip (k_twoview_lm, k_homography_lm, k_fundamental_lm):
pure numpy, deterministic, no GPU.  tests/test_twoview_edge_scenes.py checks the oracle on them, alone, and
tests/test_twoview_edge_scenes_gpu.py the device against the oracle and against tests/twoview_lm_ref.py.

Every scene is generated from the residual's definition: choose the pose (w, t), the H or the F; sample 3-D points in front of
both cameras; project; add noise.  Conventions (asserted by the CPU test: the independent residual vanishes on the noise-free
data): camera 1 is [I | 0]; camera 2 has the world-to-camera rotation R(w) and the position t, so x2 ~ R (X - t); the
angular scenes are in normalised coordinates, the homography and fundamental scenes in pixels (K below).

What the scenes reach in twoview_lm.hip:
  * correspondence counts below the number of parameters and at the wave tails 63 / 64 / 65, 127 / 128 / 129, and 0;
  * positions at and next to +-e3 (both branches of householder3's sigma <= DBL_EPSILON, beta = 0 and beta = 2), and in the
    southern hemisphere (the x[2] <= 0 form of vp);
  * rotations exactly 0, of norm 5e-9 (first-order branch of aa_to_rot), 1e-7 (just outside it) and of angle pi - 1e-3;
  * a start from which some residuals are clamped to 1000 (zero Jacobian rows) and the others are not;
  * H0 scaled by 1e+-8, negated, with H(2, 2) = 0, and singular; F0 negated, scaled, of rank 3 and rank 1, with nearly equal
    singular values, and zero.
Every case exists with the estimator's own iteration count (15; 2 and 12 for F) and as "@1" (max_num_iterations = 1).
AT_ONE_ONLY names the cases whose full-length run is chaotic -- the oracle alone moves by more than a tenth of the device
tolerance when its correspondences are permuted, or when each coordinate moves by one unit in the last place -- and that
therefore run as "@1" only; the CPU test asserts that the list is exactly that set.  The second probe is there because the
first is blind where a sum does not depend on its order: one or two correspondences (a + b = b + a exactly), or all but
one or two residuals cut off by the TRUNCATED loss (adding zeros is exact).  The list holds the exactly or nearly
interpolating problems (as many correspondences as unknowns or fewer: the final cost is round-off, and its relative
deviation means nothing) and one CGNR run that zig-zags along a valley for all 15 iterations."""
import numpy as np

TRIVIAL, HUBER, TRUNCATED = 0, 1, 6
EXACT, CGNR = 0, 1                                         # THEIA_TWO_VIEW_EXACT, THEIA_TWO_VIEW_CGNR
K = np.array([[800.0, 0.0, 400.0], [0.0, 800.0, 300.0], [0.0, 0.0, 1.0]])
PERMUTATION_SEED = 0x7E57


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1.0 - np.cos(th)) / (th * th) * (Kx @ Kx)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _points(rng, n, R, t, off_axis=0.0):
    """n points in front of both cameras, at least off_axis away from the first camera's optical axis (in the image)"""
    out = []
    while len(out) < n:
        X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 8.0)])
        if (R @ (X - t))[2] > 1.0 and np.hypot(X[0], X[1]) >= off_axis * X[2]:
            out.append(X)
    return np.array(out).reshape(n, 3)


def _project(X, R, t, Kmat, rng, noise):
    """[n][4] = (x1, y1, x2, y2) of cameras [I | 0] and R [I | -t] with calibration Kmat"""
    Y = (X - t) @ R.T
    x1 = (X / X[:, 2:]) @ Kmat.T
    x2 = (Y / Y[:, 2:]) @ Kmat.T
    c = np.hstack([x1[:, :2], x2[:, :2]])
    return c + noise * rng.standard_normal(c.shape) if noise else c


class Case:
    """kind: "angular" | "homography" | "fundamental"; x0: [6] pose or [3][3]; clean: the noise-free correspondences and
    the model they satisfy (None where the scene has none)."""
    def __init__(self, kind, corr, x0, loss=TRIVIAL, width=1.0, solver=EXACT, iters=15, clean=None, truth=None):
        self.kind, self.corr, self.x0 = kind, np.ascontiguousarray(corr, dtype=np.float64).reshape(-1, 4), np.array(x0, dtype=np.float64)
        self.loss, self.width, self.solver, self.iters, self.clean, self.truth = loss, width, solver, iters, clean, truth

    @property
    def n(self):
        return len(self.corr)

    def set_options(self, o, iters=None):
        o.max_num_iterations = self.iters if iters is None else iters
        o.loss_function_type = self.loss
        o.robust_loss_width = self.width
        return o

    def permuted(self):
        """the same problem with its correspondences in a fixed permuted order"""
        perm = np.random.default_rng(PERMUTATION_SEED + self.n).permutation(self.n)
        return Case(self.kind, self.corr[perm], self.x0, self.loss, self.width, self.solver, self.iters)

    def nudged(self):
        """the same problem with every coordinate one unit in the last place up"""
        return Case(self.kind, np.nextafter(self.corr, np.inf), self.x0, self.loss, self.width, self.solver, self.iters)

    def at(self, iters):
        return Case(self.kind, self.corr, self.x0, self.loss, self.width, self.solver, iters, self.clean, self.truth)


# ------------------------------------------------------------------ angular
ANGULAR_LOSSES = (("trivial", TRIVIAL, 1.0), ("huber", HUBER, 1e-5), ("truncated", TRUNCATED, 2e-4))
ANGULAR_COUNTS = (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129)
GENERIC_POSE = (np.array([0.12, -0.2, 0.07]), unit([0.8, 0.1, 0.45]))
_Z_AXIS_PI = (np.pi - 1e-3) * unit([0.02, -0.01, 1.0])
# name: (start rotation, start position, true rotation - start rotation, true position - start position (before normalisation))
ANGULAR_POSES = {
    "pole+":     (np.array([0.05, -0.08, 0.03]), np.array([0.0, 0.0, 1.0]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.0)),
    "pole-":     (np.array([0.05, -0.08, 0.03]), np.array([0.0, 0.0, -1.0]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.0)),
    "nearpole+": (np.array([0.05, -0.08, 0.03]), unit([1e-9, 0.0, 1.0]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.0)),
    "nearpole-": (np.array([0.05, -0.08, 0.03]), unit([1e-9, 0.0, -1.0]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.0)),
    "south":     (np.array([0.05, -0.08, 0.03]), np.array([0.6, 0.0, -0.8]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.002)),
    "rot0":      (np.zeros(3), unit([0.8, 0.1, 0.45]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.002)),
    "rot5e-9":   (5e-9 * unit([1.0, -2.0, 0.5]), unit([0.8, 0.1, 0.45]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.002)),
    "rot1e-7":   (1e-7 * unit([1.0, -2.0, 0.5]), unit([0.8, 0.1, 0.45]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.002)),
    "rotpi":     (_Z_AXIS_PI, unit([0.8, 0.1, 0.45]), (0.002, -0.003, 0.001), (0.004, -0.003, 0.002)),
}
# large enough that a residual (~ noise^2) is well above the cancellation in a / 2 - sqrt(a^2 / 4 - b^2): the costs are then
# conditioned well enough for a relative comparison
ANGULAR_NOISE = 5e-3


def angular_scene(seed, n, w_true, t_true, noise=ANGULAR_NOISE, off_axis=0.0):
    """The reference's a = f1.(M f1) + (R f2).(M R' f2) pairs R f2 with R' f2: next to the poles, where M removes the
    optical axis, it is negative for a point near the axis, and the residual is then a and not 0 on exact data.  off_axis
    keeps the points of those scenes away from it."""
    rng = np.random.default_rng(seed)
    R = rodrigues(w_true)
    X = _points(rng, n, R, t_true, off_axis)
    clean = _project(X, R, t_true, np.eye(3), rng, 0.0)
    return clean + noise * rng.standard_normal(clean.shape), clean


def _angular_cases():
    out = {}

    def add(label, corr, x0, clean, truth):
        for sname, solver in (("exact", EXACT), ("cgnr", CGNR)):
            losses = ANGULAR_LOSSES if len(corr) >= 5 else ANGULAR_LOSSES[2:]
            for lname, loss, width in losses:
                out[f"angular/{label}/{sname}/{lname}"] = Case("angular", corr, x0, loss, width, solver, 15, clean, truth)

    w, t = GENERIC_POSE
    x0 = np.concatenate([w + np.array([0.003, -0.002, 0.004]), unit(t + np.array([0.005, -0.004, 0.003]))])
    for n in ANGULAR_COUNTS:
        corr, clean = angular_scene(0xA000 + n, n, w, t)
        add(f"n{n}", corr, x0, clean, np.concatenate([w, t]))
    for k, (name, (w0, t0, dw, dt)) in enumerate(ANGULAR_POSES.items()):
        wt, tt = w0 + np.array(dw), unit(t0 + np.array(dt))
        corr, clean = angular_scene(0xA100 + k, 65, wt, tt, off_axis=0.15 if "pole" in name else 0.0)
        add(name, corr, np.concatenate([w0, t0]), clean, np.concatenate([wt, tt]))
    # started at the pole with a turn of 0.6 about the optical axis: 40 correspondences of a pose next to the start and 25 of
    # the generic pose, far from it.  For some of the latter the square root's argument is negative at the start (residual
    # 1000, zero Jacobian row); the former keep the problem well conditioned under every loss
    w0, t0 = np.array([0.0, 0.0, 0.6]), np.array([0.0, 0.0, 1.0])
    wt, tt = w0 + np.array([0.002, -0.003, 0.001]), unit(t0 + np.array([0.004, -0.003, 0.0]))
    near, near_clean = angular_scene(0xA200, 40, wt, tt, off_axis=0.15)
    far, far_clean = angular_scene(0xA201, 25, w, t)
    add("clamped-mix", np.vstack([near, far]), np.concatenate([w0, t0]), near_clean, np.concatenate([wt, tt]))
    return out


# ------------------------------------------------------------------ homography
HOMOGRAPHY_LOSSES = (("trivial", TRIVIAL, 1.0), ("truncated", TRUNCATED, 50.0))
HOMOGRAPHY_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 129)
PIXEL_NOISE = 0.5


def true_homography():
    """K (R + t n' / d) K^-1 of a plane in front of both cameras, H(2, 2) = 1"""
    R = rodrigues([0.03, -0.05, 0.02])
    H = K @ (R + np.outer([0.3, -0.1, 0.2], [0.1, -0.05, 1.0]) / 5.0) @ np.linalg.inv(K)
    return H / H[2, 2]


def homography_scene(seed, n, noise=PIXEL_NOISE):
    rng = np.random.default_rng(seed)
    H = true_homography()
    x1 = np.column_stack([rng.uniform(0.0, 800.0, n), rng.uniform(0.0, 600.0, n), np.ones(n)]).reshape(n, 3)
    p = x1 @ H.T
    clean = np.hstack([x1[:, :2], p[:, :2] / p[:, 2:]])
    return clean + noise * rng.standard_normal(clean.shape), clean


def _homography_cases():
    out = {}
    Ht = true_homography()
    H0 = Ht * 1.3 + np.array([[0.01, -0.01, 2.0], [0.01, 0.0, -2.0], [1e-6, 0.0, 0.0]])
    Hz = H0.copy(); Hz[2, 2] = 0.0
    starts = {"typical": H0, "x1e8": H0 * 1e8, "x1e-8": H0 * 1e-8, "negated": -H0, "h22zero": Hz,
              "singular": np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])}       # determinant exactly 0

    def add(label, corr, x0, clean):
        for lname, loss, width in HOMOGRAPHY_LOSSES:
            out[f"homography/{label}/{lname}"] = Case("homography", corr, x0, loss, width, EXACT, 15, clean, Ht)

    for n in HOMOGRAPHY_COUNTS:
        corr, clean = homography_scene(0xB000 + n, n)
        add(f"n{n}", corr, H0, clean)
    for k, (name, Hs) in enumerate(starts.items()):
        if name != "typical":
            corr, clean = homography_scene(0xB100 + k, 65)
            add(name, corr, Hs, clean)
    return out


# ------------------------------------------------------------------ fundamental matrix
FUNDAMENTAL_COUNTS = (0, 1, 2, 6, 7, 8, 63, 64, 65, 129)
FUNDAMENTAL_ITERS = (2, 12)


def fundamental_of(w, t, Kmat=K):
    """F with x2' F x1 = 0 for cameras Kmat [I | 0] and Kmat R(w) [I | -t], Frobenius norm 1"""
    R = rodrigues(w)
    t = np.asarray(t, dtype=np.float64)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(Kmat)
    F = Ki.T @ R @ tx @ Ki                                  # E = R [t]x: (R (X - t))' R [t]x X = 0
    return F / np.linalg.norm(F)


FUNDAMENTAL_POSE = (np.array([0.04, -0.12, 0.03]), np.array([1.0, 0.1, 0.2]))
FUNDAMENTAL_START = (FUNDAMENTAL_POSE[0] + np.array([0.004, -0.003, 0.002]), FUNDAMENTAL_POSE[1] + np.array([0.01, -0.02, 0.015]))


def fundamental_scene(seed, n, Kmat=K, noise=PIXEL_NOISE):
    """noise in pixels of K, whatever Kmat is"""
    rng = np.random.default_rng(seed)
    w, t = FUNDAMENTAL_POSE
    R = rodrigues(w)
    X = _points(rng, n, R, t)
    clean = _project(X, R, t, Kmat, rng, 0.0)
    return clean + noise * Kmat[0, 0] / K[0, 0] * rng.standard_normal(clean.shape), clean


def _fundamental_cases():
    """The starts with coinciding singular values are in NORMALISED coordinates (Kmat = I), where they occur: an essential
    matrix has the singular values (1, 1, 0).  In pixels such an F0 is nowhere near a fundamental matrix of the data."""
    out = {}
    I3 = np.eye(3)
    F0 = fundamental_of(*FUNDAMENTAL_START)
    E0 = fundamental_of(*FUNDAMENTAL_START, Kmat=I3)
    U, S, Vt = np.linalg.svd(F0)
    Ue, Se, Vte = np.linalg.svd(E0)
    starts = {"typical": (F0, K), "negated": (-F0, K), "x1e6": (F0 * 1e6, K),
              "fullrank": (F0 + 1e-3 * S[0] * np.outer(U[:, 2], Vt[2]), K),
              "rank1": (np.outer(Ue[:, 0], Vte[0]), I3),
              "nearequal": (Ue @ np.diag([1.0, 0.999, 0.0]) @ Vte, I3),
              "zero": (np.zeros((3, 3)), K)}

    def add(label, corr, x0, clean, Kmat):
        for it in FUNDAMENTAL_ITERS:
            out[f"fundamental/{label}/it{it}"] = Case("fundamental", corr, x0, TRIVIAL, 1.0, EXACT, it, clean, fundamental_of(*FUNDAMENTAL_POSE, Kmat=Kmat))

    for n in FUNDAMENTAL_COUNTS:
        corr, clean = fundamental_scene(0xC000 + n, n)
        add(f"n{n}", corr, F0, clean, K)
    for k, (name, (Fs, Kmat)) in enumerate(starts.items()):
        if name != "typical":
            corr, clean = fundamental_scene(0xC100 + k, 65, Kmat)
            add(name, corr, Fs, clean, Kmat)
    return out


FULL = {}
FULL.update(_angular_cases())
FULL.update(_homography_cases())
FULL.update(_fundamental_cases())


def base_of(name):
    """the "@1" form's key: a fundamental case has one "@1" form for its two iteration counts"""
    parts = name.split("/")
    return "/".join(parts[:-1]) if parts[0] == "fundamental" else name


# full-length runs that the oracle alone does not reproduce under a permutation of the correspondences or a nudge of one
# unit in the last place (see the module docstring); asserted to be exactly that set by test_twoview_edge_scenes.py::test_at_one_only_is_exactly_the_unadmitted_set
AT_ONE_ONLY = (
    "angular/n2/exact/truncated",
    "angular/n3/cgnr/truncated",
    "angular/n4/exact/truncated",
    "angular/n4/cgnr/truncated",
    "angular/n5/exact/trivial",
    "angular/n5/exact/huber",
    "angular/n5/exact/truncated",
    "angular/n5/cgnr/trivial",
    "angular/n5/cgnr/huber",
    "angular/n5/cgnr/truncated",
    "angular/rot1e-7/cgnr/trivial",
    "angular/rot1e-7/cgnr/truncated",
    "homography/n1/trivial",
    "homography/n1/truncated",
    "homography/n2/trivial",
    "homography/n2/truncated",
    "homography/n3/trivial",
    "homography/n3/truncated",
    "homography/n4/trivial",
    "homography/n4/truncated",
    "fundamental/n2/it12",
    "fundamental/n6/it12",
)

# the fundamental starts whose singular values coincide (or nearly): the tangent basis of the manifold is not unique there,
# so the independent step of tests/twoview_lm_ref.py is not compared; device versus oracle still is.  Nothing else belongs here.
NO_UNIQUE_BASIS = ("fundamental/rank1", "fundamental/nearequal", "fundamental/zero")

CASES = {}
for _name, _case in FULL.items():
    if _name not in AT_ONE_ONLY:
        CASES[_name] = _case
    CASES.setdefault(base_of(_name) + "@1", _case.at(1))
del _name, _case


def has_unique_basis(name):
    return not any(name.startswith(p) for p in NO_UNIQUE_BASIS)


def n_params(kind):
    return {"angular": 5, "homography": 9, "fundamental": 7}[kind]


# ------------------------------------------------------------------ running and comparing
POSE_TOL, ANGULAR_COST_TOL = 1e-9, 1e-9                   # absolute; relative (test_two_views_angular_batch_follows_oracle)
MATRIX_TOL, MATRIX_COST_TOL = 1e-8, 1e-8                  # relative to the largest entry; relative (test_optimize_*_batch_*)
# the first step against tests/twoview_lm_ref.py: ten times the largest deviation of the ORACLE measured by
# test_twoview_edge_scenes.py (its docstring has the figures); the pose absolute, H and F relative to their largest entry
STEP_BOUND = {"angular": 2e-11, "homography": 5e-12, "fundamental": 4.3e-12}
INITIAL_COST_BOUND = 3.2e-11                               # relative, against the numpy.longdouble sum
COUNTS = ("num_iterations", "num_successful_steps", "termination_type", "success")
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


def solve_oracle(case):
    """(result, summary dict) of the CPU oracle on one case"""
    from tests import oracle_lib as ol
    o = case.set_options(ol.default_options())
    with np.errstate(all="ignore"):
        if case.kind == "angular":
            return ol.two_views_angular(case.corr, case.x0, o, case.solver)
        if case.kind == "homography":
            return ol.optimize_homography(case.corr, case.x0, o)
        return ol.optimize_fundamental(case.corr, case.x0, o)


def _cost_deviation(g, r, tol):
    if not np.isfinite(r):
        return 0.0 if (np.isnan(g) and np.isnan(r)) or g == r else np.inf
    if g == r:
        return 0.0
    return abs(g - r) / (tol * abs(r)) if r != 0.0 else np.inf


def deviations(case, got, ref):
    """got, ref = (result, summary dict).  Returns (counts equal, {quantity: deviation in units of its tolerance})."""
    (xg, sg), (xr, sr) = got, ref
    same = all(sg[k] == sr[k] for k in COUNTS)
    xg, xr = np.asarray(xg, dtype=np.float64), np.asarray(xr, dtype=np.float64)
    if np.array_equal(xg, xr, equal_nan=True):
        dx = 0.0
    elif not np.all(np.isfinite(xr)):
        dx = np.inf                                                          # a failed or degenerate result: the same bits
    elif case.kind == "angular":
        dx = np.abs(xg - xr).max() / POSE_TOL
    else:
        dx = np.abs(xg - xr).max() / (MATRIX_TOL * np.abs(xr).max())
    ctol = ANGULAR_COST_TOL if case.kind == "angular" else MATRIX_COST_TOL
    return same, {"x": float(dx), "initial_cost": _cost_deviation(sg["initial_cost"], sr["initial_cost"], ctol),
                  "final_cost": _cost_deviation(sg["final_cost"], sr["final_cost"], ctol)}
