"""CPU: the K3 test systems (tests/k3_systems.py) and their yardsticks, and the argument checks of the K3 introspection
entries (the library is loaded, no device is touched)."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from tests import k3_systems as ks


def tile_pattern(M, n, tol=0.0):
    nt = ks.num_tiles(n)
    P = np.zeros((nt, nt), bool)
    for I in range(nt):
        for J in range(nt):
            P[I, J] = np.abs(M[np.ix_(ks.tile_cols(n, I), ks.tile_cols(n, J))]).max() > tol
    return P


@pytest.mark.parametrize("n, adj", [(130, ks.path(3)), (64 * 8 - 5, ks.ring(8)), (64 * 9, ks.star(9, 4)),
                                    (64 * 12 - 63, ks.random_graph(12, 3, 7))])
def test_generator_is_spd_with_the_declared_tile_pattern(n, adj):
    s = ks.make_system(n, adj, seed=n)
    assert np.array_equal(s.A, s.A.T)
    np.linalg.cholesky(s.A)
    assert np.array_equal(tile_pattern(s.A, n), (adj != 0) | np.eye(ks.num_tiles(n), dtype=bool))


def test_generator_conditioning_follows_the_column_scaling():
    kap = [ks.make_system(64 * 8, ks.ring(8), 3, cscale=c).ref()[1] for c in (0, 2, 4)]
    assert 1e2 < kap[0] < 1e8 and kap[0] < kap[1] < kap[2] and kap[2] > 1e11


def test_generator_ranks_sum_to_the_system_and_private_tiles_stay_home():
    n, R = 64 * 12 - 5, 3
    s = ks.make_system(n, ks.ring(12), 11, num_ranks=R, rank_of=lambda tiles, rng: (tiles[0] * R) // 12)
    assert np.abs(s.parts_A.sum(axis=0) - s.A).max() <= 1e-13 * np.abs(s.A).max()
    assert np.array_equal(s.parts_b.sum(axis=0), s.b)
    cls = s.tile_class
    assert (cls == 1).any() and (cls == 0).any()
    for t in range(s.nt):
        c = cls[:, t]
        assert (c == 0).all() or ((c == 1).sum() == 1 and (c == 2).sum() == R - 1)
    for r in range(R):
        pat = tile_pattern(s.parts_A[r], n)
        for t in np.nonzero(cls[r] == 2)[0]:       # another rank's tile: nothing of it here
            assert not pat[t].any() and not pat[:, t].any()
            assert not s.parts_b[r][ks.tile_cols(n, t)].any()


@pytest.mark.parametrize("cscale", [0.0, 2.0, 4.0])
def test_lapack_meets_the_eta_bound(cscale):
    s = ks.make_system(64 * 6 - 17, ks.band(6, 2), 5, cscale=cscale)
    x, kappa, eta_lapack = s.ref()
    assert eta_lapack <= ks.eta_bound(s.n)
    assert ks.eta(s.A, x, s.b) <= eta_lapack
    L = ks.tile_cholesky(s.A)
    xt = ks.solve_with_factor(L, s.b)
    assert ks.eta(s.A, xt, s.b) <= ks.eta_bound(s.n)
    assert ks.forward_error(xt, x) <= ks.fwd_bound(s.n, kappa)


@pytest.mark.parametrize("skip", [(0, 1, 1), (1, 2, 2), (2, 3, 3), (0, 2, 1), (3, 4, 4)])
def test_a_dropped_tile_update_misses_the_eta_bound_by_1e6(skip):
    """The bound can see the errors the GPU tests are there to catch: one tile update left out of the factorisation."""
    n = 64 * 5 - 3
    adj = ks.adj_from_edges(5, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2)])
    s = ks.make_system(n, adj, 2)
    L = ks.tile_cholesky(s.A, skip=skip)
    assert ks.eta(s.A, ks.solve_with_factor(L, s.b), s.b) >= 1e6 * ks.eta_bound(n)


def test_factor_structure_of_a_ring_closes_the_cycle():
    adj = ks.ring(5)
    phys, edges = ks.factor_structure(adj, [0, 1, 2, 3, 4])
    assert phys[4, 1] and phys[4, 2] and phys[4, 3] and not phys[2, 0]
    assert (1, 4) in edges and (3, 4) in edges


def _solve_rc(n, lda, adj, mode):
    A = np.zeros((max(n, 1), max(lda, 1))); b = np.zeros(max(n, 1)); x = np.zeros(max(n, 1))
    a = None if adj is None else np.ascontiguousarray(adj, np.uint8)
    return capi.lib().theia_hip_tile_sparse_spd_solve(n, lda, capi.ptr(a, C.c_uint8), mode, capi.ptr(A, C.c_double),
                                                      capi.ptr(b, C.c_double), capi.ptr(x, C.c_double), None, None, None)


def test_tile_sparse_entry_refuses_bad_arguments_before_the_device():
    bad = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert _solve_rc(130, 129, ks.path(3), 0) == bad            # lda < n
    assert _solve_rc(0, 0, None, 0) == bad
    assert _solve_rc(130, 130, ks.path(3), 3) == bad             # mode
    asym = ks.path(3).copy(); asym[0, 1] = 0
    assert _solve_rc(130, 130, asym, 0) == bad
    assert b"symmetric" in capi.lib().theia_hip_last_error()


def test_sharded_entry_refuses_inconsistent_tile_classes_before_the_device():
    n, R = 64 * 4, 2
    adj = np.ascontiguousarray(ks.ring(4))
    A = np.zeros((R, n, n)); b = np.zeros((R, n)); x = np.zeros((R, n))
    info = (capi.K3Info * R)()

    def rc(cls, a=adj):
        cls = np.ascontiguousarray(cls, np.uint8)
        return capi.lib().theia_hip_tile_sparse_spd_solve_sharded(n, R, capi.ptr(np.ascontiguousarray(a, np.uint8), C.c_uint8),
                                                                  capi.ptr(cls, C.c_uint8), capi.ptr(A, C.c_double),
                                                                  capi.ptr(b, C.c_double), capi.ptr(x, C.c_double), info)
    bad = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert rc([[1, 1, 0, 0], [1, 2, 0, 0]]) == bad     # tile 0 private to both ranks
    assert rc([[1, 2, 0, 0], [2, 2, 0, 0]]) == bad     # tile 1 private to nobody
    assert rc([[0, 2, 0, 0], [2, 1, 0, 0]]) == bad     # tile 0 shared on one rank only
    assert rc([[3, 2, 0, 0], [2, 1, 0, 0]]) == bad     # no such class
    asym = ks.ring(4).copy(); asym[1, 2] = 0
    assert rc([[1, 2, 0, 0], [2, 1, 0, 0]], asym) == bad
