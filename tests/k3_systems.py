"""BA-like SPD systems with an exact 64 x 64 tile structure, and the high-precision yardsticks of the K3 tests.

S = sum of v v^T over "tracks": a track is supported on 3 - 12 random columns of one tile, or of the two tiles of a
declared edge, so the non-zero tile pattern of S is exactly the declared adjacency plus the diagonal tiles.  An LM-style
diagonal mu * diag(S) + delta makes it SPD; optional column scaling 10^U(-c, c) spreads the conditioning.  Tracks can be
dealt to ranks: rank r's partial system S_r sums its own tracks, and sum_r S_r = S (the distributed BA's shape).

Yardsticks: the normwise backward error eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), residual in long double, and
the forward error against x_ref (LAPACK FP64, refined twice with long-double residuals).
"""
import numpy as np
import scipy.linalg as sla

NB = 64
U = 2.0 ** -53
ETA_C = 8.0        # eta bound: ETA_C * u * sqrt(n), independent of the conditioning (measured: <= 1 u at n = 1, <= 0.06 u sqrt(n) beyond)
FWD_C = 8.0        # forward error bound: FWD_C * kappa_inf * (eta bound)


def num_tiles(n):
    return (n + NB - 1) // NB


def tile_cols(n, t):
    return np.arange(t * NB, min(n, (t + 1) * NB))


def eta_bound(n):
    return ETA_C * U * np.sqrt(n)


# ---------------------------------------------------------------- tile graphs (symmetric 0/1, zero diagonal)
def adj_from_edges(nt, edges):
    a = np.zeros((nt, nt), np.uint8)
    for i, j in edges:
        if i != j:
            a[i, j] = a[j, i] = 1
    return a


def path(nt):
    return adj_from_edges(nt, [(i, i + 1) for i in range(nt - 1)])


def ring(nt):
    return adj_from_edges(nt, [(i, (i + 1) % nt) for i in range(nt)])


def star(nt, center=0):
    return adj_from_edges(nt, [(center, j) for j in range(nt) if j != center])


def band(nt, width):
    return adj_from_edges(nt, [(i, i + d) for i in range(nt) for d in range(1, width + 1) if i + d < nt])


def grid(rows, cols):
    e = []
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols:
                e.append((r * cols + c, r * cols + c + 1))
            if r + 1 < rows:
                e.append((r * cols + c, (r + 1) * cols + c))
    return adj_from_edges(rows * cols, e)


def complete(nt):
    return adj_from_edges(nt, [(i, j) for i in range(nt) for j in range(i)])


def path_with_chords(nt, chords):
    return adj_from_edges(nt, [(i, i + 1) for i in range(nt - 1)] + list(chords))


def disjoint(*graphs):
    """Block-diagonal union of tile graphs (components in the given order)."""
    nt = sum(g.shape[0] for g in graphs)
    a = np.zeros((nt, nt), np.uint8)
    o = 0
    for g in graphs:
        k = g.shape[0]
        a[o:o + k, o:o + k] = g
        o += k
    return a


def intrinsics_ring(nt, hubs=2):
    """Tiles [0, hubs) couple to every tile (the shared-intrinsics columns); the camera tiles [hubs - 1, nt) form a ring."""
    e = [(h, j) for h in range(hubs) for j in range(nt) if j != h]
    cams = list(range(hubs - 1, nt))
    e += [(cams[i], cams[(i + 1) % len(cams)]) for i in range(len(cams))]
    return adj_from_edges(nt, e)


def random_graph(nt, mean_degree, seed):
    rng = np.random.default_rng(seed)
    m = int(round(nt * mean_degree / 2))
    e = set()
    while len(e) < m:
        i, j = rng.integers(0, nt, 2)
        if i != j:
            e.add((min(i, j), max(i, j)))
    return adj_from_edges(nt, sorted(e))


def edges_of(adj):
    i, j = np.nonzero(np.tril(adj, -1))
    return list(zip(i.tolist(), j.tolist()))


# ---------------------------------------------------------------- systems
class System:
    """A (n x n, both triangles), b; with ranks: parts_A [R][n][n], parts_b [R][n], tile_class [R][nt]."""

    def __init__(self, n, adj, A, b, parts_A=None, parts_b=None, tile_class=None, scale=None):
        self.n, self.adj, self.A, self.b = n, adj, A, b
        self.parts_A, self.parts_b, self.tile_class, self.scale = parts_A, parts_b, tile_class, scale
        self._ref = None

    @property
    def nt(self):
        return num_tiles(self.n)

    def ref(self):
        """(x_ref, kappa_inf, eta of LAPACK's own solve)."""
        if self._ref is None:
            self._ref = reference(self.A, self.b)
        return self._ref


def _tracks(n, adj, rng):
    """Column supports of the tracks: (cols, tiles touched)."""
    nt = num_tiles(n)
    out = []
    for t in range(nt):
        for _ in range(3):               # every column of the tile in three tracks
            cols = rng.permutation(tile_cols(n, t))
            o = 0
            while o < len(cols):
                k = int(rng.integers(3, 13))
                out.append((np.sort(cols[o:o + k]), (t,)))
                o += k
    for i, j in edges_of(adj):
        for _ in range(2):
            ci, cj = tile_cols(n, i), tile_cols(n, j)
            k = int(rng.integers(3, 13))
            ki = int(rng.integers(1, k))
            ki = min(ki, len(ci)); kj = min(max(1, k - ki), len(cj))
            cols = np.concatenate([rng.choice(ci, ki, replace=False), rng.choice(cj, kj, replace=False)])
            out.append((np.sort(cols), (i, j)))
    return out


def make_system(n, adj, seed, cscale=0.0, mu=1e-2, num_ranks=0, rank_of=None):
    """rank_of(tiles, rng) -> rank of a track (tiles: the one or two tiles it touches), with num_ranks > 0."""
    rng = np.random.default_rng(seed)
    nt = num_tiles(n)
    adj = np.asarray(adj, np.uint8)
    assert adj.shape == (nt, nt)
    R = max(1, num_ranks)
    S = np.zeros((R, n, n))
    touch = np.zeros((R, nt), bool)
    for cols, tiles in _tracks(n, adj, rng):
        v = rng.standard_normal(len(cols))
        r = int(rank_of(tiles, rng)) if num_ranks else 0
        S[r][np.ix_(cols, cols)] += np.outer(v, v)
        touch[r, list(tiles)] = True
    d = 10.0 ** rng.uniform(-cscale, cscale, n) if cscale else np.ones(n)
    S *= d[None, :, None] * d[None, None, :]
    Ssum = S.sum(axis=0)
    dg = Ssum.diagonal()
    damp = mu * dg + 1e-6 * np.median(dg)
    b = rng.standard_normal(n) * np.sqrt(dg + damp)
    A = Ssum + np.diag(damp)
    if not num_ranks:
        return System(n, adj, A, b, scale=d)
    # tile classes: shared when two or more ranks' tracks touch the tile; the diagonal and the rhs of a private column
    # go to its owner, those of a shared column to rank 0
    cls = np.zeros((R, nt), np.uint8)
    owner = np.zeros(n, int)
    for t in range(nt):
        who = np.nonzero(touch[:, t])[0]
        if len(who) == 1:
            cls[:, t] = 2
            cls[who[0], t] = 1
            owner[tile_cols(n, t)] = who[0]
    parts_b = np.zeros((R, n))
    for r in range(R):
        sel = owner == r
        S[r][sel, sel] += damp[sel]
        parts_b[r][sel] = b[sel]
    return System(n, adj, A, b, parts_A=S, parts_b=parts_b, tile_class=cls, scale=d)


# ---------------------------------------------------------------- yardsticks
def residual_ld(A, x, b, rows=512):
    """b - A x in long double (A: both triangles)."""
    n = len(b)
    xl = np.asarray(x, np.longdouble)
    r = np.empty(n, np.longdouble)
    for i0 in range(0, n, rows):
        r[i0:i0 + rows] = np.asarray(b[i0:i0 + rows], np.longdouble) - np.asarray(A[i0:i0 + rows], np.longdouble) @ xl
    return r


def eta(A, x, b):
    """Normwise backward error (nan when x is not finite)."""
    if not np.all(np.isfinite(x)):
        return float("nan")
    r = residual_ld(A, x, b)
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def reference(A, b):
    """x_ref = LAPACK Cholesky refined twice with long-double residuals; kappa_inf (LAPACK's estimate, dpocon); the eta of
    LAPACK's unrefined solution."""
    c = sla.cho_factor(A, lower=True)
    x0 = sla.cho_solve(c, b)
    x = x0.copy()
    for _ in range(2):
        x = x + sla.cho_solve(c, np.asarray(residual_ld(A, x, b), np.float64))
    anorm = np.abs(A).sum(axis=1).max()
    rcond, info = sla.lapack.dpocon(c[0], anorm, uplo="L")
    assert info == 0
    return x, 1.0 / rcond, eta(A, x0, b)


def forward_error(x, x_ref):
    return float(np.abs(x - x_ref).max() / np.abs(x_ref).max())


def fwd_bound(n, kappa):
    return FWD_C * kappa * eta_bound(n)


# ---------------------------------------------------------------- structure helpers
def factor_structure(adj, order):
    """Lower tile pattern of the factor (declared + fill) for the elimination order `order` (tile at each position), at
    the physical lower positions, diagonal included; and the factor's edges as (tile eliminated first, later tile)."""
    nt = len(order)
    L = np.zeros((nt, nt), bool)
    for I in range(nt):
        for J in range(I):
            L[I, J] = adj[order[I], order[J]] != 0
    edges = []
    for K in range(nt):
        s = [I for I in range(K + 1, nt) if L[I, K]]
        for a in s:
            for b_ in s:
                if b_ < a:
                    L[a, b_] = True
        edges += [(order[K], order[I]) for I in s]
    phys = np.eye(nt, dtype=bool)
    for K in range(nt):
        for I in range(K + 1, nt):
            if L[I, K]:
                p, q = max(order[I], order[K]), min(order[I], order[K])
                phys[p, q] = True
    return phys, edges


def poison(A, struct, n, lda=None, value=np.nan):
    """n x lda copy of A's lower triangle with `value` everywhere else: the strict upper triangle, the lower entries
    outside the tiles marked in `struct` [nt][nt] (physical lower positions), and the padding columns."""
    lda = lda or n
    nt = num_tiles(n)
    P = np.full((n, lda), value)
    for I in range(nt):
        for J in range(I + 1):
            if struct[I, J]:
                ci, cj = tile_cols(n, I), tile_cols(n, J)
                P[np.ix_(ci, cj)] = A[np.ix_(ci, cj)]
    for i in range(n):
        P[i, i + 1:] = value
    return P


def tile_cholesky(A, skip=None):
    """Right-looking tile Cholesky in natural order (numpy), the lower factor; skip = (K, I, J): leave out the update of
    tile (I, J) by source column K -- a dropped tile update, for the metric's sensitivity check."""
    n = A.shape[0]
    nt = num_tiles(n)
    L = np.tril(A).copy()
    for K in range(nt):
        k = tile_cols(n, K)
        L[np.ix_(k, k)] = np.linalg.cholesky(L[np.ix_(k, k)])
        Lkk = L[np.ix_(k, k)]
        for I in range(K + 1, nt):
            i = tile_cols(n, I)
            L[np.ix_(i, k)] = sla.solve_triangular(Lkk, L[np.ix_(i, k)].T, lower=True).T
        for I in range(K + 1, nt):
            for J in range(K + 1, I + 1):
                if skip == (K, I, J):
                    continue
                i, j = tile_cols(n, I), tile_cols(n, J)
                L[np.ix_(i, j)] -= L[np.ix_(i, k)] @ L[np.ix_(j, k)].T
    return np.tril(L)


def solve_with_factor(L, b):
    y = sla.solve_triangular(L, b, lower=True)
    return sla.solve_triangular(L.T, y, lower=False)
