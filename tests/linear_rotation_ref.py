"""numpy restatement of LinearRotationEstimator::EstimateRotations (global_pose_estimation/
linear_rotation_estimator.cc:76-204 with sfm/pose/util.cc:117-129; Martinec & Pajdla), written from the reference's
description:

  M          per pair e = (i, j): +I on the diagonal blocks (i, i) and (j, j), -R_e^T at block (i, j), -R_e at (j, i),
             R_e = AngleAxisToRotationMatrix(rotation_2); repeated pairs add up                      (:90-150)
  solution   the eigenvectors of the three smallest eigenvalues, X [3n][3]                           (:170-182)
  per view   ProjectToRotationMatrix(X_i) = U V^T of the SVD, negated when its determinant is negative, as angle-axis
                                                                                                    (:188-201)

`reference` takes the eigenvectors from np.linalg.eigh.  `device_steps` follows theia_hip_linear_rotations
(csrc/linear_rotations.hip) step by step instead: the shift mu = 3n eps max diag M, one Cholesky of M + mu I, the hashed
start block, and per iteration Y = (M + mu I)^-1 X, Q = two passes of modified Gram-Schmidt over Y's columns,
d = |Q - X (X^T Q)|_F, H = X^T Y, stop when d <= threshold.  Both index the views that have edges compactly, in view
order, and give a result that is defined up to one common rotation on the right (X_i = R_i Q / sqrt(n))."""
import numpy as np
import scipy.linalg as sla

from tests.rotation_averaging_ref import aa_to_R, R_to_aa

EPS = np.finfo(np.float64).eps


def system_views(num_views, edges):
    """The views that have an edge, in view order, and the map view -> index in the system (-1: none)."""
    edges = np.asarray(edges).reshape(-1, 2)
    has = np.zeros(num_views, dtype=bool)
    has[edges.ravel()] = True
    views = np.nonzero(has)[0]
    idx = np.full(num_views, -1)
    idx[views] = np.arange(len(views))
    return views, idx


def build_M(num_views, edges, rel):
    """The dense 3n x 3n matrix over the views with edges, and those views."""
    edges = np.asarray(edges).reshape(-1, 2)
    views, idx = system_views(num_views, edges)
    n = len(views)
    R = aa_to_R(rel)
    M = np.zeros((3 * n, 3 * n))
    for (i, j), Re in zip(edges, R):
        a, b = idx[i], idx[j]
        assert a != b
        M[3 * a:3 * a + 3, 3 * a:3 * a + 3] += np.eye(3)
        M[3 * b:3 * b + 3, 3 * b:3 * b + 3] += np.eye(3)
        M[3 * a:3 * a + 3, 3 * b:3 * b + 3] -= Re.T
        M[3 * b:3 * b + 3, 3 * a:3 * a + 3] -= Re
    return M, views


def project_blocks(X):
    """ProjectToRotationMatrix of every view's 3 x 3 block of X [3n][3], as angle-axis [n][3]."""
    B = X.reshape(-1, 3, 3)
    U, _, Vt = np.linalg.svd(B)
    R = U @ Vt
    R[np.linalg.det(R) < 0.0] *= -1.0
    return R_to_aa(R)


def reference(num_views, edges, rel):
    """eigh of M: dict(views, orientations [n][3] of those views, eigenvalues (all, ascending), M)."""
    M, views = build_M(num_views, edges, rel)
    w, V = np.linalg.eigh(M)
    return dict(views=views, orientations=project_blocks(V[:, :3]), eigenvalues=w, M=M)


def start_block(n3):
    """X0[r][k] = (((uint32)((3 r + k + 1) * 2654435761u)) >> 8) * 2^-23 - 1."""
    i = 3 * np.arange(n3, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :] + np.uint64(1)
    h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def gram_schmidt_twice(Y):
    """Modified Gram-Schmidt over the three columns in column order, two passes."""
    Q = np.array(Y, dtype=np.float64)
    for _ in range(2):
        for k in range(3):
            for j in range(k):
                Q[:, k] -= (Q[:, j] @ Q[:, k]) * Q[:, j]
            Q[:, k] /= np.linalg.norm(Q[:, k])
    return Q


def shift_of(M):
    return (M.shape[0] * EPS) * M.diagonal().max()


def device_steps(num_views, edges, rel, threshold=1e-10, max_num_iterations=1000):
    """The device algorithm: dict(views, orientations, d (one per iteration), iterations, converged, eigenvalues (the
    three, ascending, shift subtracted), shift)."""
    M, views = build_M(num_views, edges, rel)
    n3 = M.shape[0]
    mu = shift_of(M)
    factor = sla.cho_factor(M + mu * np.eye(n3), lower=True)
    X = gram_schmidt_twice(start_block(n3))
    d, H, converged = [], np.zeros((3, 3)), False
    while len(d) < max_num_iterations and not converged:
        Y = sla.cho_solve(factor, X)
        Q = gram_schmidt_twice(Y)
        d.append(float(np.linalg.norm(Q - X @ (X.T @ Q))))
        H = X.T @ Y
        X = Q
        converged = d[-1] <= threshold
    theta = np.linalg.eigvalsh(0.5 * (H + H.T))
    return dict(views=views, orientations=project_blocks(X), d=d, iterations=len(d), converged=converged,
                eigenvalues=np.sort(1.0 / theta - mu), shift=mu)


def relative_to_first(aa):
    """R_i R_0^T [n][3][3]: free of the common rotation on the right."""
    R = aa_to_R(aa)
    return R @ R[0].T


def gauge_free_angles(a, b):
    """The angle (rad) between R_i R_0^T of a and of b, per view."""
    from tests.rotation_scenes import _angle_of
    return _angle_of(relative_to_first(a) @ np.transpose(relative_to_first(b), (0, 2, 1)))
