"""numpy restatement of the LiGT position estimator (Cai et al., "A Pose-only Solution to Visual Reconstruction and
Navigation"; the stage behind theia_hip_ligt_positions), written from the algorithm and following the library's order
rules (include/theia_hip.h): tracks and observations in the caller's order, the first maximal base pair in
lexicographic (i, j) order under a strict `>` from 0, a track of fewer than three observations or without a positive
theta^2 skipped, the held view = v1 of the first track used, the other views indexed v1, v2, v3 per constraint in
(track, observation) order, every entry of H summed in (track, observation) order.

    theta^2_ij = |[f_j]x R_j R_i' f_i|^2
    per observation (v2, f2) of a used track but the one of v1, with R31 = R_v1 R_v3', R32 = R_v2 R_v3':
        a32 = ([R32 f3]x f2)' [f2]x,  C = [f1]x R31 f3 a32' R_v2,  B = |[f2]x R32 f3|^2 [f1]x R_v1,  D = -(B + C)
        H += [B C D]' [B C D] on the blocks of (v1, v2, v3); the held view's rows and columns are dropped
    positions = the unit eigenvector of H's smallest eigenvalue; the view pairs vote on its sign
"""
import numpy as np


def rotation_matrix(w):
    """Rodrigues, with ceres' first-order branch for a tiny angle."""
    w = np.asarray(w, dtype=np.float64)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th2 = float(w @ w)
    if th2 <= np.finfo(float).eps:
        return np.eye(3) + K
    th = np.sqrt(th2)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th2) * (K @ K)


def skew(f):
    return np.array([[0.0, -f[2], f[1]], [f[2], 0.0, -f[0]], [-f[1], f[0], 0.0]])


def theta_sq(f_i, f_j, R_i, R_j):
    return float(np.sum((skew(f_j) @ (R_j @ R_i.T) @ f_i) ** 2))


def base_pair(feats, Rs):
    """(i, j, best theta^2, second-best theta^2) of one track; i = -1 when no pair has a positive theta^2."""
    best, second, bi, bj = 0.0, 0.0, -1, -1
    n = len(feats)
    for i in range(n):
        for j in range(i + 1, n):
            th = theta_sq(feats[i], feats[j], Rs[i], Rs[j])
            if th > best:
                second, best, bi, bj = best, th, i, j
            elif th > second:
                second = th
    return bi, bj, best, second


def constraint(f1, f2, f3, R1, R2, R3):
    R31, R32 = R1 @ R3.T, R2 @ R3.T
    a32 = (skew(R32 @ f3) @ f2) @ skew(f2)
    C = np.outer(skew(f1) @ (R31 @ f3), a32) @ R2
    B = float(np.sum((skew(f2) @ (R32 @ f3)) ** 2)) * (skew(f1) @ R1)
    return B, C, -(B + C)


def constraint_abs(f1, f2, f3, R1, R2, R3):
    """B, C, D of constraint() with every operand replaced by its magnitude and every subtraction by an addition: the
    quantity that bounds, times a small multiple of eps, the rounding error of ANY order of evaluating them from the
    features and the rotation matrices' entries (themselves rounded).  It does not shrink where the cross products
    cancel (a small parallax between v2 and v3), where the restatement's own B, C, D are no more accurate than that."""
    f1, f2, f3, R1, R2, R3 = (np.abs(x) for x in (f1, f2, f3, R1, R2, R3))
    A = lambda f: np.abs(skew(f))
    R31, R32 = R1 @ R3.T, R2 @ R3.T
    a32 = (A(R32 @ f3) @ f2) @ A(f2)
    C = np.outer(A(f1) @ (R31 @ f3), a32) @ R2
    B = float(np.sum((A(f2) @ (R32 @ f3)) ** 2)) * (A(f1) @ R1)
    return B, C, B + C


def estimate(orientations, track_offsets, obs_view, obs_feature, edges=None, relative_translations=None):
    """Returns a dict: base_pairs [T][2] (-1 -1 skipped), theta_gap [T] = (best - second) / best of the used tracks (nan
    otherwise), index [n] (-1 held, -2 not in the system), H and abs_sum [3 (m - 1)]^2 (per entry the sum of the
    magnitudes of its contributions, a contribution being every product of magnitudes that the entry is a signed sum of:
    H assembled from constraint_abs), eigenvalues (ascending, of H), vector (the unit eigenvector of the smallest), positions
    [n][3] after the sign vote (zeros outside the system), estimated [n], votes, flipped, constraints."""
    aa = np.asarray(orientations, dtype=np.float64).reshape(-1, 3)
    off = np.asarray(track_offsets, dtype=np.int64)
    ov = np.asarray(obs_view, dtype=np.int64)
    fe = np.column_stack([np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2), np.ones(len(ov))])
    n, T = aa.shape[0], len(off) - 1
    R = np.array([rotation_matrix(w) for w in aa])
    base = np.full((T, 2), -1, dtype=np.int32)
    gap = np.full(T, np.nan)
    index = np.full(n, -2, dtype=np.int32)
    m = 0
    triplets = []   # (v1, v2, v3, B, C, D) in (track, observation) order
    constraints = 0
    for t in range(T):
        o0, L = off[t], off[t + 1] - off[t]
        if L < 3:
            continue
        views = ov[o0:o0 + L]
        bi, bj, best, second = base_pair(fe[o0:o0 + L], R[views])
        if bi < 0:
            continue
        base[t] = (bi, bj)
        gap[t] = (best - second) / best
        v1, v3 = views[bi], views[bj]
        for k in range(L):
            if k == bi:
                continue
            v2 = views[k]
            for v in (v1, v2, v3):
                if index[v] == -2:
                    index[v] = m - 1
                    m += 1
            constraints += 1
            if k == bj:     # the observation of v3 itself: B = C = D = 0
                continue
            args = (fe[o0 + bi], fe[o0 + k], fe[o0 + bj], R[v1], R[v2], R[v3])
            triplets.append((v1, v2, v3) + constraint(*args) + constraint_abs(*args))
    out = dict(base_pairs=base, theta_gap=gap, index=index, constraints=constraints, num_views_in_system=m)
    if m == 0:
        return out
    k3 = 3 * (m - 1)
    H = np.zeros((k3, k3))
    A = np.zeros((k3, k3))
    for v1, v2, v3, B, C, D, Ba, Ca, Da in triplets:
        vs, Ms, As = (v1, v2, v3), (B, C, D), (Ba, Ca, Da)
        for a in range(3):
            for b in range(3):
                ia, ib = index[vs[a]], index[vs[b]]
                if ia < 0 or ib < 0:
                    continue
                P = Ms[a].T @ Ms[b]
                H[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3] += P
                A[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3] += As[a].T @ As[b]
    w, V = np.linalg.eigh(H)
    x = V[:, 0]
    pos = np.zeros((n, 3))
    est = index != -2
    for v in range(n):
        if index[v] >= 0:
            pos[v] = x[3 * index[v]:3 * index[v] + 3]
    votes = 0
    if edges is not None:
        for (a, b), t12 in zip(np.asarray(edges).reshape(-1, 2), np.asarray(relative_translations).reshape(-1, 3)):
            if not (est[a] and est[b]):
                continue
            d = pos[b] - pos[a]
            nrm = np.linalg.norm(d)
            if nrm > 0:
                d = d / nrm
            votes += 1 if float((R[a] @ d) @ t12) > 0 else -1
    if votes < 0:
        pos = -pos
    out.update(H=H, abs_sum=A, eigenvalues=w, vector=x, positions=pos, estimated=est, votes=votes, flipped=votes < 0)
    return out
