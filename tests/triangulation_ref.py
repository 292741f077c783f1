"""Plain references for the triangulation stage of theia_hip_estimate_tracks (csrc/ba_batch.hip) and for
theia_hip_track_statistics (test side only; no device).

  * projection_matrix(): Camera::GetProjectionMatrix (camera.cc:195-200) = K [R | -R c], K from IntrinsicsToCalibrationMatrix
    (projection_matrix_utils.cc:50-58) with each model's own slots (*_camera_model.cc GetCalibrationMatrix: FOV and division
    undistortion have no skew slot, the principal point sits in slots 2 and 3 there), R the ceres angle-axis rule;
  * midpoint() / nview_l2() / nview_svd(): TriangulateMidpoint, TriangulateNView, TriangulateNViewSVD (triangulation.cc:130-214)
    in mpmath at 60 digits, each with what a per-track tolerance needs (N, ||M||_2, the gap between the two smallest
    eigenvalues; for the midpoint the condition number of its 3 x 3 matrix);
  * nview_svd_rounds(): the DEVICE's fixed-point iteration on mu restated in float64 numpy.  It chooses inputs (does a track
    settle within 24 rounds?); it is never the expected value;
  * sufficient_angle(), track_stats(): SufficientTriangulationAngle (triangulation.cc:236-250) and the three sweeps of
    SetOutlierTracksToUnestimated in numpy, the projection itself taken from the oracle.

C_NP: the largest ratio error / (N eps ||M|| / gap) (midpoint: error / (N eps cond)) that float64 numpy (eigh, svd, solve)
shows against the mpmath value over all the cuts of tests/triangulation_scenes.py, rounded up.  test_triangulation_ref.py
asserts that the measured figures stay below them; the device is allowed 10 * max(C_NP, 1) (it sums in another order, uses
cyclic Jacobi instead of LAPACK, and stops mu at 1e-13 relative)."""
import functools

import mpmath
import numpy as np

from tests import ba_edge_scenes as es

mp = mpmath.mp
DPS = 60
EPS = float(np.finfo(np.float64).eps)
NO_SKEW_MODELS = (3, 4)     # THEIA_CAM_FOV, THEIA_CAM_DIVISION_UNDISTORTION

# measured: see test_triangulation_ref.test_references_agree_and_numpy_constants (the figures are in its docstring)
C_NP = {"l2": 1.0, "svd": 1.0, "midpoint": 1.0}


def device_c(kind):
    return 10.0 * max(C_NP[kind], 1.0)


# ---------------------------------------------------------------- projection matrix
def rotation_matrix(w):
    """ceres::AngleAxisRotatePoint as a matrix: Rodrigues if theta^2 > DBL_EPSILON, else the first-order I + [w]x."""
    w = np.asarray(w, dtype=np.float64)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    t2 = float(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if t2 > EPS:
        t = np.sqrt(t2)
        return np.eye(3) + (np.sin(t) / t) * W + ((1.0 - np.cos(t)) / t2) * (W @ W)
    return np.eye(3) + W


def calibration_matrix(model, k):
    f, a = k[0], k[1]
    if int(model) in NO_SKEW_MODELS:
        s, cx, cy = 0.0, k[2], k[3]
    else:
        s, cx, cy = k[2], k[3], k[4]
    return np.array([[f, s, cx], [0.0, f * a, cy], [0.0, 0.0, 1.0]])


def projection_matrix(model, k, ext):
    ext = np.asarray(ext, dtype=np.float64)
    R = rotation_matrix(ext[3:6])
    return calibration_matrix(model, k) @ np.column_stack([R, -R @ ext[:3]])


def track_inputs(p, t):
    """(projection matrices [N][3][4], pixels [N][2], camera centres [N][3], observation rows) of track t of a FlatProblem."""
    sel = np.flatnonzero(p.obs_pt == t)
    Ps = np.array([projection_matrix(p.group_model[p.cam_group[c]], p.intrinsics[p.cam_group[c]], p.cam_ext[c]) for c in p.obs_cam[sel]]).reshape(-1, 3, 4)
    return Ps, p.obs_uv[sel], p.cam_ext[p.obs_cam[sel], :3], sel


# ---------------------------------------------------------------- mpmath
def _mpm(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a.reshape(a.shape[0], -1)])


def _two_smallest(M):
    """(lambda0, lambda1, unit eigenvector of lambda0) of a symmetric positive semidefinite mp matrix.  Up to 16 rows by the
    full decomposition; beyond that by inverse iteration on one LU factorisation (the second pair deflated against the first)."""
    n = M.rows
    if n <= 16:
        E, Q = mp.eigsy(M)
        order = sorted(range(n), key=lambda i: E[i])
        return E[order[0]], E[order[1]], Q[:, order[0]]
    LU, piv = mp.LU_decomp(M)
    solve = lambda b: mp.U_solve(LU, mp.L_solve(LU, b, piv))
    found = []
    for start in range(2):
        v = mp.matrix([mp.mpf(1) / (1 + ((7 * i + 3 * start) % 11)) for i in range(n)])
        lam = mp.mpf(0)
        for it in range(400):
            for u in found:
                v = v - u * (u.T * v)[0]
            v = solve(v)
            for u in found:
                v = v - u * (u.T * v)[0]
            v = v / mp.norm(v)
            new = (v.T * (M * v))[0]
            done = abs(new - lam) <= mp.mpf(10) ** (-(DPS - 12 if start == 0 else 12)) * abs(new)    # (lambda1 only scales a tolerance)
            lam = new
            if done and it >= 2:
                break
        else:
            raise RuntimeError("inverse iteration did not converge")
        found.append(v)
        if start == 0:
            lam0 = lam
    return lam0, lam, found[0]


def _vec(v):
    return np.array([float(x) for x in v])


def midpoint(origins, dirs):
    """TriangulateMidpoint: sum (I - d d^T) X = sum (I - d d^T) o.  -> dict(X [3] or None when the matrix is singular, N, cond)."""
    with mp.workdps(DPS):
        A = mp.zeros(3, 3); b = mp.zeros(3, 1)
        for o, d in zip(np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64)):
            dm = _mpm(d.reshape(3, 1)); T = mp.eye(3) - dm * dm.T
            A += T; b += T * _mpm(o.reshape(3, 1))
        E = sorted(mp.eigsy(A, eigvals_only=True))
        if E[0] <= 0:
            return {"X": None, "N": len(dirs), "cond": float("inf")}
        return {"X": _vec(mp.lu_solve(A, b)), "N": len(dirs), "cond": float(E[2] / E[0])}


def _result(M, lam0, lam1, v, N, head=None):
    norm = float(np.linalg.norm(np.array(M.tolist(), dtype=np.float64), 2))     # (a scale of the tolerance: float64 is enough)
    x = _vec(v)
    return {"x": x if head is None else x[:head], "N": N, "norm": norm, "gap": float(lam1 - lam0), "lambda": float(lam0)}


def l2_matrix(Ps, pixels):
    M = np.zeros((4, 4))
    for P, uv in zip(Ps, pixels):
        n = np.array([uv[0], uv[1], 1.0]); n /= np.linalg.norm(n)
        Cm = P - np.outer(n, n @ P)
        M += Cm.T @ Cm
    return M


def svd_matrix(Ps, pixels):
    N = len(Ps)
    A = np.zeros((3 * N, 4 + N))
    for i, (P, uv) in enumerate(zip(Ps, pixels)):
        A[3 * i:3 * i + 3, :4] = -P
        A[3 * i:3 * i + 3, 4 + i] = [uv[0], uv[1], 1.0]
    return A


def nview_l2(Ps, pixels):
    """TriangulateNView: the unit eigenvector of the smallest eigenvalue of M = sum C^T C, C = (I - n n^T) P."""
    with mp.workdps(DPS):
        M = mp.zeros(4, 4)
        for P, uv in zip(Ps, pixels):
            x = mp.matrix([mp.mpf(float(uv[0])), mp.mpf(float(uv[1])), mp.mpf(1)])
            n = x / mp.norm(x)
            Pm = _mpm(P)
            Cm = Pm - n * (n.T * Pm)
            M += Cm.T * Cm
        lam0, lam1, v = _two_smallest(M)
        return _result(M, lam0, lam1, v, len(Ps))


def nview_svd(Ps, pixels):
    """TriangulateNViewSVD: the first four entries of the unit right singular vector of the smallest singular value of
    A = [-P_i | e_i x_i], taken as the smallest eigenvector of M = A^T A."""
    with mp.workdps(DPS):
        A = _mpm(svd_matrix(Ps, pixels))
        M = A.T * A
        lam0, lam1, v = _two_smallest(M)
        return _result(M, lam0, lam1, v, len(Ps), head=4)


def sign_error(got, ref):
    """|got -+ ref|_2, the smaller of the two signs."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(min(np.linalg.norm(got - ref), np.linalg.norm(got + ref)))


def eigen_tolerance(ref, c):
    return c * ref["N"] * EPS * ref["norm"] / ref["gap"] if ref["gap"] > 0.0 else float("inf")


def midpoint_tolerance(ref, c):
    return c * ref["N"] * EPS * ref["cond"]


# ---------------------------------------------------------------- float64 restatements
def numpy_l2(Ps, pixels):
    return np.linalg.eigh(l2_matrix(Ps, pixels))[1][:, 0]


def numpy_svd(Ps, pixels):
    return np.linalg.svd(svd_matrix(Ps, pixels))[2][-1][:4]


def numpy_midpoint(origins, dirs):
    A = np.zeros((3, 3)); b = np.zeros(3)
    for o, d in zip(origins, dirs):
        T = np.eye(3) - np.outer(d, d)
        A += T; b += T @ o
    return np.linalg.solve(A, b)


def nview_svd_rounds(Ps, pixels, max_rounds=24, strict=False):
    """The device's iteration (triangulate_nview, svd): D(mu) = sum C^T C - mu (I + sum t t^T / (d - mu)), t = n^T P, mu <- the
    Rayleigh quotient of the full vector, until |dmu| <= 1e-13 mu, or until the steps have stopped shrinking below 1e-10 mu (the
    rounding floor of mu: a Rayleigh quotient of residuals of about a pixel between numbers of about 1e3 is good to a few 1e-13,
    and the iteration then alternates between two neighbouring values for ever).  strict: the first rule alone, which the kernel
    had before that floor was found.  -> (rounds used, settled, x [4] scaled to unit norm over all 4 + N entries, the L2 vector of
    the first round)."""
    Ps = np.asarray(Ps, dtype=np.float64); pixels = np.asarray(pixels, dtype=np.float64)
    xs = np.column_stack([pixels, np.ones(len(pixels))])
    d = (xs ** 2).sum(1)
    n = xs / np.sqrt(d)[:, None]
    t = np.einsum("ni,nij->nj", n, Ps)
    Cm = Ps - n[:, :, None] * t[:, None, :]
    M0 = np.einsum("nri,nrj->ij", Cm, Cm)
    mu, x_l2, dmu_prev = 0.0, None, np.inf
    for rnd in range(max_rounds):
        D = M0.copy()
        if mu != 0.0:
            D -= np.einsum("n,ni,nj->ij", mu / (d - mu), t, t) + mu * np.eye(4)
        x = np.linalg.eigh(D)[1][:, 0]
        if rnd == 0:
            x_l2 = x.copy()
        px = Ps @ x
        lam = np.einsum("ni,ni->n", xs, px) / (d - mu)
        e = px - lam[:, None] * xs
        den = x @ x + lam @ lam
        mu_new = (e ** 2).sum() / den
        dmu = abs(mu_new - mu)
        settled = dmu <= 1e-13 * mu_new or mu_new == mu or (not strict and dmu <= 1e-10 * mu_new and dmu >= dmu_prev)
        mu, dmu_prev = mu_new, dmu
        if settled or rnd == max_rounds - 1:
            return rnd + 1, bool(settled), x / np.sqrt(den), x_l2
    raise AssertionError


# ---------------------------------------------------------------- angle test and statistics
def sufficient_angle(dirs, deg):
    """SufficientTriangulationAngle: some pair of rays with cos(angle) < cos(deg)."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    if len(d) < 2:
        return False
    return bool(np.any(np.triu(d @ d.T < np.cos(np.deg2rad(deg)), 1)))


def track_stats(p):
    """(mean squared reprojection error, views behind the camera, minimum ray cosine, smallest |depth| / |X - w C|) per track of p
    at p.points.  The projection is the oracle's; the depth is (R (X - w C))_z / w (Camera::ProjectPoint), the rays are
    X.hnormalized() - C (SufficientTriangulationAngle as SetOutlierTracksToUnestimated calls it); 2.0 below two views."""
    npts = p.points.shape[0]
    ok, uv = es.project_with_oracle(p, p.cam_ext, p.points)
    r2 = ((uv - p.obs_uv) ** 2).sum(1)
    cnt = np.bincount(p.obs_pt, minlength=npts)
    with np.errstate(invalid="ignore", divide="ignore"):
        mse = np.bincount(p.obs_pt, weights=r2, minlength=npts) / cnt
    X = p.points[p.obs_pt]
    q = X[:, :3] - X[:, 3:4] * p.cam_ext[p.obs_cam, :3]
    R = np.stack([rotation_matrix(c[3:]) for c in p.cam_ext])
    depth = np.einsum("nj,nj->n", R[p.obs_cam, 2, :], q) / X[:, 3]
    behind = np.bincount(p.obs_pt, weights=(depth < 0.0), minlength=npts).astype(np.int32)
    margin = np.abs(depth * X[:, 3]) / np.linalg.norm(q, axis=1)
    rays = X[:, :3] / X[:, 3:4] - p.cam_ext[p.obs_cam, :3]
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    mincos = np.full(npts, 2.0)
    for t in range(npts):
        d = rays[p.obs_pt == t]
        if len(d) >= 2:
            G = d @ d.T
            mincos[t] = G[np.triu_indices(len(d), 1)].min()
    return ok, mse, behind, mincos, margin


# ---------------------------------------------------------------- per scene, computed once
@functools.lru_cache(maxsize=None)
def cut_references(model, variant="cut"):
    """{track: {"l2": ..., "svd": ...}} of the tracks of a cut with two observations or more (mpmath; about a second for the
    65-observation track)."""
    from tests import triangulation_scenes as ts
    p = ts.variant(model, variant).p
    out = {}
    for t in range(p.points.shape[0]):
        Ps, uv, _, sel = track_inputs(p, t)
        if len(sel) >= 2:
            out[t] = {"l2": nview_l2(Ps, uv), "svd": nview_svd(Ps, uv)}
    return out


def midpoint_references(p, rays):
    """{track: midpoint()} of the tracks with two observations or more, on the given rays."""
    out = {}
    for t in range(p.points.shape[0]):
        sel = np.flatnonzero(p.obs_pt == t)
        if len(sel) >= 2:
            out[t] = midpoint(p.cam_ext[p.obs_cam[sel], :3], rays[sel])
    return out
