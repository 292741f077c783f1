"""CPU: the oracle's copies of the team solvers' algorithms (EISPACK orthes + hqr2, the 9 x 9 Jacobi SVD, five-point steps
1-3) on the families of tests/team_solver_cases.py, against the 40-digit mpmath yardstick.  The oracle runs the same code
as the device routines, so this checks the shared algorithm itself without a GPU; tests/test_team_solvers_gpu.py checks
that the teams equal it bit for bit."""
import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import team_solver_cases as tc


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", tc.REF_N)
@pytest.mark.parametrize("family", tc.EIG_FAMILIES)
def test_oracle_eig_families_against_mpmath(family, n, cplx):
    A = tc.eig_matrix(family, n)
    ok, wr, wi, H, V = tc.eig_oracle(A, cplx)
    if family in tc.NONFINITE:
        # n >= 3: the QR sweep runs on NaN to the iteration bound and gives up; n <= 2 has no sweep: the roots come out
        # non-finite instead (EISPACK and Eigen alike)
        assert not ok if n >= 3 else not (np.all(np.isfinite(wr)) and np.all(np.isfinite(wi)))
        return
    assert ok, f"{family} n={n}: the eigen-solver gave up"
    worst = tc.eig_accuracy(A, wr, wi, V, cplx, tc.eig_reference(family, n), family in tc.DEFECTIVE)
    assert worst <= 1.0, f"{family} n={n}: error / bound = {worst:.3g}"


@pytest.mark.parametrize("n", [1, 2, 3, 4, 10])
def test_oracle_eig_zero_matrix(n):
    """The zero matrix: eigenvalues 0 and V = I (before the guard, n >= 3 ran the QR sweep on 0 / 0 to the iteration bound
    and n = 2 rotated V by 0 / 0)."""
    for cplx in (False, True):
        ok, wr, wi, H, V = tc.eig_oracle(np.zeros((n, n)), cplx)
        assert ok and np.array_equal(wr, np.zeros(n)) and np.array_equal(wi, np.zeros(n))
        assert np.array_equal(V, np.eye(n)) and np.array_equal(H, np.zeros((n, n)))


@pytest.mark.parametrize("kind", sorted(tc.ACTION_N))
def test_oracle_eig_action_matrices_against_mpmath(kind):
    ref = tc.eig_reference(("action", kind, 0), None)
    A = ref[0]
    ok, wr, wi, _, V = tc.eig_oracle(A, True)
    assert ok
    worst = tc.eig_accuracy(A, wr, wi, V, True, ref, False)
    assert worst <= 1.0, f"{kind}: error / bound = {worst:.3g}"
    if A.shape[0] <= 10:   # the real-only instantiation takes the same decisions
        ok0, wr0, wi0, _, V0 = tc.eig_oracle(A, False)
        assert ok0 and np.array_equal(wr0, wr) and np.array_equal(wi0, wi)
        real = wi == 0.0
        assert np.array_equal(V0[:, real], V[:, real])


@pytest.mark.parametrize("n", [8, 13, 27])
def test_oracle_eig_gauss_at_production_sizes(n):
    A = tc.eig_matrix("gauss", n)
    ok, wr, wi, _, V = tc.eig_oracle(A, True)
    assert ok
    worst = tc.eig_accuracy(A, wr, wi, V, True, tc.eig_reference("gauss", n), False)
    assert worst <= 1.0, worst


def test_eig_accuracy_rejects_a_wrong_eigenvalue():
    """The yardstick has teeth: one eigenvalue moved by 1e-12 relative misses the bound."""
    A = tc.eig_matrix("gauss", 10)
    ok, wr, wi, _, V = tc.eig_oracle(A, True)
    wr = wr.copy()
    j = int(np.argmax(wi == 0.0))
    wr[j] *= 1.0 + 1e-12
    assert tc.eig_accuracy(A, wr, wi, V, True, tc.eig_reference("gauss", 10), False) > 1.0


@pytest.mark.parametrize("family", tc.SVD_FAMILIES)
def test_oracle_svd9_against_mpmath(family):
    A = tc.svd_matrix(family)
    Uo, S, Vo = ol.svd9(A)
    worst = tc.svd_accuracy(A, Uo, S, Vo, tc.svd_reference(family))
    assert worst <= 1.0, f"{family}: error / bound = {worst:.3g}"


@pytest.mark.parametrize("family", tc.FP_FAMILIES)
def test_oracle_five_point_pre_rank_and_null_space(family):
    for seed in range(4):
        corr = tc.fp_corr(family, seed)
        ok, N, M = tc.five_point_pre_oracle(corr)
        assert ok == (tc.exact_rank(tc.fp_system(corr)) == 5), (family, seed)
        if ok:
            assert tc.fp_null_ratio(corr, N) <= 1.0
            # the last four rows of the action matrix are the fixed -1 pattern
            assert M[6, 0] == M[7, 1] == M[8, 3] == M[9, 6] == -1.0
