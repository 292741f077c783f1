"""numpy restatement of the linear triplet position estimator (Jiang, Cui, Tan, "A Global Linear Method for Camera Pose
Registration", ICCV 2013; the stage behind theia_hip_linear_triplet_positions), written from the algorithm and the
library's stated rules (include/theia_hip.h), not from the device code:

    triangles (a < b < c) of the view pairs in lexicographic order
    per triangle and per track seen by all three views: unit rays f = (x, y, 1) / |.|; for each of the pairs (a, b),
      (a, c), (b, c) the directions d0 = f_first, d1 = R_2' f_second must satisfy d0 . d1 < cos(2 deg); the midpoint p
      solves ((I - d0 d0') + (I - d1 d1')) p = (I - d1 d1') position_2 by LLT (a non-positive pivot skips the track);
      depths |p| and |p - position_2|; ratios d1_12 / d1_13 and d2_12 / d2_23, both finite and positive or the track is
      skipped; baseline = (1, the rank k / 2 element of the first ratios, the rank k / 2 element of the second)
    a triangle without a valid track is dropped (state 1); the remaining triangles are grouped by shared edges, the
      largest group is used (state 0; ties: the group of the first triangle), the others are state 2
    counts, view index (a, b, c over the used triangles; the first view held, -1) and w = 1 / sqrt(min count)
    three constraint rows per triangle, H = sum C' C without the held view, the eigenvector of the smallest eigenvalue,
      the pairs' sign vote
"""
import numpy as np

EPS = np.finfo(float).eps
COS_MIN_ANGLE = float(np.cos(np.deg2rad(2.0)))
# roundings charged to one midpoint: the ray's normalisation, R_2' f, the two outer products, the right-hand side, the
# 3 x 3 factorisation and its two substitutions, the norm of the result -- 32 eps of the operands' magnitudes covers
# each side, and the comparison is between two such evaluations
RATIO_EPS = 64.0 * EPS


def rotation_matrix(w):
    """Rodrigues, with ceres' first-order branch for a tiny angle."""
    w = np.asarray(w, dtype=np.float64)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th2 = float(w @ w)
    if th2 <= EPS:
        return np.eye(3) + K
    th = np.sqrt(th2)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th2) * (K @ K)


def find_triplets(num_views, edges):
    """All (a < b < c, edge ab, edge ac, edge bc) in lexicographic order."""
    up = [dict() for _ in range(num_views)]
    for e, (i, j) in enumerate(np.asarray(edges).reshape(-1, 2)):
        up[int(i)][int(j)] = e
    out = []
    for a in range(num_views):
        for b in sorted(up[a]):
            for c in sorted(up[b]):
                if c in up[a]:
                    out.append((a, b, c, up[a][b], up[a][c], up[b][c]))
    return out


def midpoints(d0, d1, o1):
    """Vectorised over tracks: d0, d1 [k][3] unit directions from the origins 0 and o1.  Returns (ok [k], depth at the
    first origin, depth at the second, |p|-relative error bound of p per unit of RATIO_EPS handled by the caller)."""
    k = d0.shape[0]
    I = np.eye(3)
    A = (I - d0[:, :, None] * d0[:, None, :]) + (I - d1[:, :, None] * d1[:, None, :])
    b = o1[None, :] - d1 * (d1 @ o1)[:, None]
    ok = np.ones(k, dtype=bool)
    L = np.zeros((k, 3, 3))
    with np.errstate(all="ignore"):
        for j in range(3):
            piv = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
            ok &= piv > 0.0
            L[:, j, j] = np.sqrt(np.where(piv > 0.0, piv, 1.0))
            for i in range(j + 1, 3):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
        y = np.zeros((k, 3))
        for i in range(3):
            y[:, i] = (b[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
        p = np.zeros((k, 3))
        for i in (2, 1, 0):
            p[:, i] = (y[:, i] - (L[:, i + 1:, i] * p[:, i + 1:]).sum(axis=1)) / L[:, i, i]
        dep0 = np.linalg.norm(p, axis=1)
        dep1 = np.linalg.norm(p - o1[None, :], axis=1)
        c = (d0 * d1).sum(axis=1)
        # |dp| <= |A^-1| (|db| + |dA| |p|) <= 2 / (1 - c^2) (|o1| + 2 |p|) per unit rounding: A's eigenvalues are 2,
        # 1 + c and 1 - c, its entries lie in [-2, 2] and b's in [-|o1|, |o1|]
        dp = 2.0 / (1.0 - c * c) * (np.linalg.norm(o1) + 2.0 * dep0)
    return ok, dep0, dep1, dp


def from_two_vectors(a, b):
    """Eigen's Quaternion::FromTwoVectors(a, b).toRotationMatrix(), and its magnitude version (every term of every
    entry replaced by its magnitude).  The antiparallel case (c < -1 + 1e-12) is the rotation by pi about
    u = normalize(v0 x e_k), k the first component of v0 of smallest magnitude.  Third value: the margin of that choice,
    second smallest minus smallest magnitude (inf outside the branch)."""
    v0, v1 = a / np.linalg.norm(a), b / np.linalg.norm(b)
    c = float(v1 @ v0)
    if c < -1.0 + 1e-12:
        mags = np.abs(v0)
        k = int(np.argmin(mags))   # argmin returns the first minimum
        e = np.zeros(3); e[k] = 1.0
        u = np.cross(v0, e)
        u = u / np.linalg.norm(u)
        srt = np.sort(mags)
        return 2.0 * np.outer(u, u) - np.eye(3), 2.0 * np.outer(np.abs(u), np.abs(u)) + np.eye(3), float(srt[1] - srt[0])
    axis = np.cross(v0, v1)
    s = np.sqrt((1.0 + c) * 2.0)
    x, y, z = axis / s
    w = s * 0.5
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                  [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    A = np.abs(np.array([[1.0 + (tyy + tzz), abs(txy) + abs(twz), abs(txz) + abs(twy)],
                         [abs(txy) + abs(twz), 1.0 + (txx + tzz), abs(tyz) + abs(twx)],
                         [abs(txz) + abs(twy), abs(tyz) + abs(twx), 1.0 + (txx + tyy)]]))
    return R, A, float("inf")


def constraint_rows(r012, r201, r120, base, w):
    """The three rows [C0 C1 C2] of one triangle."""
    I = np.eye(3)
    s012, s201, s120 = base[0] / base[2], base[1] / base[0], base[2] / base[1]
    m2 = -2.0 * w * I
    return [[(-s201 * r201 + r012.T / s012 + I) * w, (s201 * r201 - r012.T / s012 + I) * w, m2],
            [(-r201.T / s201 + s120 * r120 + I) * w, m2, (r201.T / s201 - s120 * r120 + I) * w],
            [m2, (-s012 * r012 + r120.T / s120 + I) * w, (s012 * r012 - r120.T / s120 + I) * w]]


def constraint_rows_abs(a012, a201, a120, base, w):
    I = np.eye(3)
    s012, s201, s120 = base[0] / base[2], base[1] / base[0], base[2] / base[1]
    m2 = 2.0 * w * I
    p0 = (s201 * a201 + a012.T / s012 + I) * w
    p1 = (a201.T / s201 + s120 * a120 + I) * w
    p2 = (s012 * a012 + a120.T / s120 + I) * w
    return [[p0, p0, m2], [p1, m2, p1], [m2, p2, p2]]


def inverse_iteration(H, threshold=1e-8, max_iterations=1000):
    """The library's iteration on H + mu I, mu = n eps max diag H, from x = 1 / sqrt(n): (iterations, x, converged)."""
    n = H.shape[0]
    mu = n * EPS * H.diagonal().max()
    Lc = np.linalg.cholesky(H + mu * np.eye(n))
    x = np.full(n, 1.0 / np.sqrt(n))
    for it in range(1, max_iterations + 1):
        y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, x))
        xn = y / np.linalg.norm(y)
        s = -1.0 if float(xn @ x) < 0.0 else 1.0
        diff = float(np.linalg.norm(xn - s * x))
        x = xn
        if diff <= threshold:
            return it, x, True
    return max_iterations, x, False


def baseline_stage(num_views, edges, relative_rotations, relative_translations, track_offsets, obs_view, obs_feature):
    """The triangles and their baseline ratios: a dict of triplets (list of (a, b, c, edge ab, edge ac, edge bc)), state
    (0, or 1 without ratios), baselines, baseline_bound, common, valid, ratios, gate_margin (see estimate)."""
    ed = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rt = np.asarray(relative_translations, dtype=np.float64).reshape(-1, 3)
    off = np.asarray(track_offsets, dtype=np.int64)
    ov = np.asarray(obs_view, dtype=np.int64)
    fe = np.column_stack([np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2), np.ones(len(ov))])
    fe = fe / np.linalg.norm(fe, axis=1)[:, None]
    n = num_views
    R2 = np.array([rotation_matrix(w) for w in np.asarray(relative_rotations, dtype=np.float64).reshape(-1, 3)])
    seen = [dict() for _ in range(n)]   # view -> {track: observation}
    for t in range(len(off) - 1):
        for o in range(off[t], off[t + 1]):
            seen[ov[o]][t] = o
    tri = find_triplets(n, ed)
    Tn = len(tri)
    state = np.zeros(Tn, dtype=np.int32)
    baselines = np.zeros((Tn, 3))
    bbound = np.zeros((Tn, 2))
    common = np.zeros(Tn, dtype=np.int64)
    valid = np.zeros(Tn, dtype=np.int64)
    ratios, margins = [], []
    for k, (a, b, c, eab, eac, ebc) in enumerate(tri):
        tracks = sorted(set(seen[a]) & set(seen[b]) & set(seen[c]))
        common[k] = len(tracks)
        if not tracks:
            state[k] = 1
            ratios.append(np.zeros((0, 2)))
            continue
        fa = fe[[seen[a][t] for t in tracks]]
        fb = fe[[seen[b][t] for t in tracks]]
        fc = fe[[seen[c][t] for t in tracks]]
        ok = np.ones(len(tracks), dtype=bool)
        res = []
        for (f0, f1, e) in ((fa, fb, eab), (fa, fc, eac), (fb, fc, ebc)):
            d1 = f1 @ R2[e]            # rows: R2' f
            dot = (f0 * d1).sum(axis=1)
            margins.append(np.abs(dot - COS_MIN_ANGLE))
            ok &= dot < COS_MIN_ANGLE
            good, dep0, dep1, dp = midpoints(f0, d1, rt[e])
            ok &= good
            res.append((dep0, dep1, dp))
        with np.errstate(all="ignore"):
            r1 = res[0][0] / res[1][0]      # depth1_12 / depth1_13
            r2 = res[0][1] / res[2][0]      # depth2_12 / depth2_23
            ok &= np.isfinite(r1) & (r1 > 0.0) & np.isfinite(r2) & (r2 > 0.0)
            e1 = RATIO_EPS * (res[0][2] / res[0][0] + res[1][2] / res[1][0])
            e2 = RATIO_EPS * (res[0][2] / res[0][1] + res[2][2] / res[2][0])
        valid[k] = int(ok.sum())
        ratios.append(np.column_stack([r1[ok], r2[ok]]))
        if valid[k] == 0:
            state[k] = 1
            continue
        mid = valid[k] // 2
        baselines[k] = (1.0, np.sort(r1[ok])[mid], np.sort(r2[ok])[mid])
        bbound[k] = (e1[ok].max(), e2[ok].max())
    return dict(triplets=tri, state=state, baselines=baselines, baseline_bound=bbound, common=common, valid=valid,
                ratios=ratios, gate_margin=np.concatenate(margins) if margins else np.zeros(0))


def estimate(orientations, edges, relative_rotations, relative_translations, track_offsets, obs_view, obs_feature):
    """Returns a dict: triplets [Tn][3], triplet_edges [Tn][3], state [Tn], baselines [Tn][3] (zeros for state 1),
    baseline_bound [Tn][2] (relative, of the two medians), common [Tn] common-track counts, valid [Tn] valid-track
    counts, ratios (list per triangle of [k][2]), gate_margin (all |d0 . d1 - cos 2 deg| of the common tracks' pairs),
    ftv_margin (the antiparallel branch's axis choices), index [n], counts, H, abs_sum, h_bound (entrywise bound of
    |H_gpu - H|), eigenvalues, vector, positions, estimated, votes, flipped, num_views_in_system."""
    aa = np.asarray(orientations, dtype=np.float64).reshape(-1, 3)
    ed = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rt = np.asarray(relative_translations, dtype=np.float64).reshape(-1, 3)
    n = aa.shape[0]
    R = np.array([rotation_matrix(w) for w in aa])
    st = baseline_stage(n, ed, relative_rotations, rt, track_offsets, obs_view, obs_feature)
    tri, state, baselines, bbound = st["triplets"], st["state"], st["baselines"], st["baseline_bound"]
    common, valid, ratios, Tn = st["common"], st["valid"], st["ratios"], len(st["triplets"])
    # components over shared edges of the surviving triangles
    parent = list(range(len(ed)))

    def root(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for k, (_, _, _, e0, e1_, e2_) in enumerate(tri):
        if state[k] == 0:
            for e in (e1_, e2_):
                ra, rb = root(e0), root(e)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    size, first = {}, {}
    for k, t in enumerate(tri):
        if state[k] == 0:
            r_ = root(t[3])
            size[r_] = size.get(r_, 0) + 1
            first.setdefault(r_, k)
    out = dict(triplets=np.array([t[:3] for t in tri], dtype=np.int32).reshape(-1, 3),
               triplet_edges=np.array([t[3:] for t in tri], dtype=np.int32).reshape(-1, 3), state=state,
               baselines=baselines, baseline_bound=bbound, common=common, valid=valid, ratios=ratios,
               gate_margin=st["gate_margin"], num_views_in_system=0)
    if not size:
        return out
    best = min(size, key=lambda r_: (-size[r_], first[r_]))
    for k, t in enumerate(tri):
        if state[k] == 0 and root(t[3]) != best:
            state[k] = 2
    used = [k for k in range(Tn) if state[k] == 0]
    counts = np.zeros(n, dtype=np.int64)
    index = np.full(n, -2, dtype=np.int32)
    m = 0
    for k in used:
        for v in tri[k][:3]:
            counts[v] += 1
            if index[v] == -2:
                index[v] = m - 1
                m += 1
    k3 = 3 * (m - 1)
    H, A, HB = np.zeros((k3, k3)), np.zeros((k3, k3)), np.zeros((k3, k3))
    ftv_margin = []
    for k in used:
        a, b, c, eab, eac, ebc = tri[k]
        w = 1.0 / np.sqrt(min(counts[a], counts[b], counts[c]))
        t01, t02, t12 = -R[a].T @ rt[eab], -R[a].T @ rt[eac], -R[b].T @ rt[ebc]
        r012, a012, m0 = from_two_vectors(t12, -t01)
        r201, a201, m1 = from_two_vectors(t01, t02)
        r120, a120, m2 = from_two_vectors(-t02, -t12)
        ftv_margin += [m0, m1, m2]
        rows = constraint_rows(r012, r201, r120, baselines[k], w)
        rows_abs = constraint_rows_abs(a012, a201, a120, baselines[k], w)
        # the s ratios carry the medians' relative errors b1, b2 (s012: b2, s201: b1, s120: b1 + b2), a product of
        # two constraint blocks twice that
        factor = 64.0 * EPS + 2.0 * (bbound[k][0] + bbound[k][1])
        vs = (a, b, c)
        for i in range(3):
            for j in range(3):
                ia, ib = index[vs[i]], index[vs[j]]
                if ia < 0 or ib < 0:
                    continue
                P = (rows[0][i].T @ rows[0][j] + rows[1][i].T @ rows[1][j]) + rows[2][i].T @ rows[2][j]
                Pa = (rows_abs[0][i].T @ rows_abs[0][j] + rows_abs[1][i].T @ rows_abs[1][j]) + rows_abs[2][i].T @ rows_abs[2][j]
                H[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3] += P
                A[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3] += Pa
                HB[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3] += factor * Pa
    wv, V = np.linalg.eigh(H)
    x = V[:, 0]
    pos = np.zeros((n, 3))
    est = index != -2
    for v in range(n):
        if index[v] >= 0:
            pos[v] = x[3 * index[v]:3 * index[v] + 3]
    votes = 0
    for (a, b), t12 in zip(ed, rt):
        if not (est[a] and est[b]):
            continue
        d = pos[b] - pos[a]
        nrm = np.linalg.norm(d)
        if nrm > 0:
            d = d / nrm
        votes += 1 if float((R[a] @ d) @ t12) > 0 else -1
    if votes < 0:
        pos = -pos
    out.update(index=index, counts=counts, H=H, abs_sum=A, h_bound=HB, eigenvalues=wv, vector=x, positions=pos,
               estimated=est, votes=votes, flipped=votes < 0, num_views_in_system=m,
               ftv_margin=np.array(ftv_margin))
    return out
