"""Numpy restatements of the reference's reconstruction alignment (src/theia/sfm/transformation/), written from its text; the
tests of pytheiasfm_amd/alignment.py and csrc/alignment*.{h,hip} compare against them.  Nothing here is derived from csrc/.

    umeyama                 AlignPointCloudsUmeyamaWithWeights (align_point_clouds.cc:56-150): sequential sums, LAPACK's SVD,
                            the degenerate rule on absolute singular values
    similarity_apply        s * (R p) + t in the library's stated order: row times vector with the products
                            added left to right, then the scale, then the translation -- elementwise numpy, so nothing is fused
    transform               TransformReconstruction (transform_reconstruction.cc:48-94) on flat arrays; orientations as matrices
    camera_alignment_fit / camera_alignment_errors   CameraAlignmentEstimator (align_reconstructions.cc:54-93), for
                            numpy_routes.ransac_replay
    align_rotations         AlignRotations (align_rotations.cc:127-156) as a Ceres-rule Levenberg-Marquardt whose residual is
                            written in torch float64 and differentiated by torch.func"""
import numpy as np

OK, DEGENERATE = 0, 1
LD = np.longdouble


def _seq_sum(x):
    """sum over axis 0, term after term as the reference's loops add"""
    return np.cumsum(np.asarray(x, dtype=np.float64), axis=0)[-1]


def umeyama(left, right, weights=None):
    """-> dict(R, t, s, status, sv): right ~ s R left + t; sv = singular values of the cross-correlation."""
    left = np.asarray(left, dtype=np.float64).reshape(-1, 3); right = np.asarray(right, dtype=np.float64).reshape(-1, 3)
    n = left.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(n)
    assert n > 0 and (w >= 0).all()
    wsum = _seq_sum(w)
    assert wsum > 0
    lc = _seq_sum(left * w[:, None]) / wsum
    rc = _seq_sum(right * w[:, None]) / wsum
    dl, dr = left - lc, right - rc
    sigma = _seq_sum((dl * dl).sum(1) * w) / wsum
    cc = _seq_sum((w[:, None] * dl)[:, :, None] * dr[:, None, :]) / wsum
    U, S, Vt = np.linalg.svd(cc.T)
    out = dict(R=np.eye(3), t=np.zeros(3), s=1.0, status=DEGENERATE, sv=S)
    if S.max() / (S.min() + 1e-12) > 1e6 or S.min() < 1e-8:
        return out
    s22 = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    s = (S[0] + S[1] + s22 * S[2]) / sigma
    R = U @ np.diag([1.0, 1.0, s22]) @ Vt
    out.update(R=R, t=rc - s * (R @ lc), s=float(s), status=OK, reflected=s22 < 0)
    return out


def similarity_apply(R, t, s, p):
    """rows of p [n][3] -> s * (R p) + t, the stated order"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = s * ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r]
    return out


def rotation_ld(w):
    """exp([w]x) for rows of w, in extended precision"""
    w = np.asarray(w, dtype=LD).reshape(-1, 3)
    t2 = (w * w).sum(1)
    th = np.sqrt(t2)
    safe = np.where(t2 > 0, th, LD(1))
    a = np.where(t2 > 0, np.sin(safe) / safe, LD(1))
    b = np.where(t2 > 0, 2 * (np.sin(safe / 2) / safe) ** 2, LD(0.5))
    K = np.zeros((len(w), 3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3, dtype=LD) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def transform(cameras, camera_estimated, points, point_estimated, R, t, s):
    """-> (cameras' [n][6] with the POSITIONS transformed and the angle-axis columns left as they were, orientation matrices
    R_cam R^T [n][3][3] in extended precision, points' [m][4]).  Unestimated rows are copies."""
    cameras = np.array(cameras, dtype=np.float64).reshape(-1, 6); points = np.array(points, dtype=np.float64).reshape(-1, 4)
    cm = np.asarray(camera_estimated, dtype=bool); pm = np.asarray(point_estimated, dtype=bool)
    cam_out, pt_out = cameras.copy(), points.copy()
    cam_out[cm, :3] = similarity_apply(R, t, s, cameras[cm, :3])
    with np.errstate(all="ignore"):
        h = points[pm, :3] / points[pm, 3:4]
    pt_out[pm, :3] = similarity_apply(R, t, s, h)
    pt_out[pm, 3] = 1.0
    orient = rotation_ld(cameras[:, 3:6])
    orient[cm] = orient[cm] @ np.asarray(R, dtype=LD).T
    return cam_out, orient, pt_out


def camera_alignment_fit(rows):
    """rows [4][6] = camera1 | camera2 -> the one model (R, t, s) of EstimateModel: Umeyama of positions2 -> positions1"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    u = umeyama(rows[:, 3:6], rows[:, 0:3])
    return u["R"], u["t"], u["s"]


def camera_alignment_errors(model, data):
    """|camera1 - (s R camera2 + t)|^2 per datum"""
    R, t, s = model
    d = np.asarray(data, dtype=np.float64).reshape(-1, 6)
    e = d[:, 0:3] - similarity_apply(R, t, s, d[:, 3:6])
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


# ------------------------------------------------------------------------------------------------ AlignRotations
def align_rotations(gt_rotation, rotation, max_num_iterations=50, function_tolerance=0.0, gradient_tolerance=1e-10,
                    parameter_tolerance=1e-8, max_trust_region_radius=1e16):
    """AlignRotations (align_rotations.cc:127-156) restated: the residual gt_i - AngleAxis(R(rotation_i) R(w)) written in torch
    float64 on the branch-by-branch maps of tests/nonlinear_rotation_ref.py (_rot, _log: ceres' AngleAxisToRotationMatrix and
    RotationMatrixToAngleAxis) and differentiated by torch.func; the dense normal equations on the host; Ceres 2.2's
    trust-region rules as tests/nonlinear_rotation_ref.py::solve plays them, with the options the reference leaves
    (function_tolerance 0).  Returns a dict: w, aligned (ApplyRotationTransformation of the input), trace [(cost, gradient max
    norm, step norm, radius, accepted)], iterations, successful, unsuccessful, invalid, term, margin (the smallest relative
    margin of a decision; the function rule at tolerance 0 is a test for equality and is left out of it)."""
    import torch
    from torch.func import jacrev, vmap
    from tests.nonlinear_rotation_ref import (_log, _rot, _margin, TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_CAP,
                                              TERM_FAILURE, TERM_RADIUS)
    gt = torch.tensor(np.asarray(gt_rotation, dtype=np.float64).reshape(-1, 3))
    rot = torch.tensor(np.asarray(rotation, dtype=np.float64).reshape(-1, 3))
    Ru = vmap(_rot)(rot)

    def aligned_of(R, w):
        return _log(R @ _rot(w))

    def residual(g, R, w):
        return g - aligned_of(R, w)
    res = vmap(residual, in_dims=(0, 0, None))
    jac = vmap(jacrev(residual, argnums=2), in_dims=(0, 0, None))

    def evaluate(w, want_jac):
        wt = torch.tensor(w)
        r = res(gt, Ru, wt).numpy().reshape(-1)
        cost = 0.5 * float((r * r).sum())
        return cost, r, (jac(gt, Ru, wt).numpy().reshape(-1, 3) if want_jac else None)
    w = np.zeros(3)
    x_cost, r, J = evaluate(w, True)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    gmax = float(np.abs(J.T @ r).max())
    x_norm = 0.0
    radius, decrease = 1e4, 2.0
    trace = [(x_cost, gmax, 0.0, radius, 1)]
    out = dict(iterations=0, successful=0, unsuccessful=0, invalid=0, margin=np.inf)
    it, invalid_run, successful, term = 0, 0, True, None

    def decide(a, b):
        out["margin"] = min(out["margin"], _margin(a, b))
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
        A = Js.T @ Js + np.diag(np.clip((Js * Js).sum(0), 1e-6, 1e32) / radius)
        try:
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
        wc = w - y * scale
        cand, rc, _ = evaluate(wc, False)
        if not np.all(np.isfinite(rc)):
            cand = np.finfo(np.float64).max
        step_norm = float(np.linalg.norm(wc - w))
        decide(step_norm, parameter_tolerance * (x_norm + parameter_tolerance))
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            trace.append((cand, gmax, step_norm, radius, 0)); term = TERM_PARAMETER; break
        change = x_cost - cand
        if abs(change) <= function_tolerance * x_cost:
            trace.append((cand, gmax, step_norm, radius, 0)); term = TERM_FUNCTION; break
        rho = change / mcc
        decide(rho, 1e-3)
        if rho > 1e-3:
            w = wc
            x_norm = float(np.linalg.norm(w))
            x_cost, r, J = evaluate(w, True)
            Js = J * scale
            gmax = float(np.abs(J.T @ r).max())
            radius = min(max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease = 2.0; successful = True
            out["successful"] += 1
            trace.append((x_cost, gmax, step_norm, radius, 1))
        else:
            radius /= decrease; decrease *= 2.0; successful = False
            out["unsuccessful"] += 1
            trace.append((cand, gmax, step_norm, radius, 0))
    if term == TERM_FAILURE:
        w = np.zeros(3)
    aligned = vmap(aligned_of, in_dims=(0, None))(Ru, torch.tensor(w)).numpy()
    out.update(w=w, aligned=aligned, trace=trace, iterations=it, term=term, radius=radius, cost=x_cost, initial_cost=trace[0][0])
    return out
