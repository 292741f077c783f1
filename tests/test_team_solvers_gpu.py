"""GPU: the team eigen, SVD and five-point routines (eig_team.h, svd_team.h, fit5_team.h) run directly, in their production
launch shapes, through the self-check entries of csrc/selftest_team_solvers.hip.  Each must equal the one-thread device
routine it replaces bit for bit, and that routine must equal the CPU oracle; the results are also held to the 40-digit
mpmath bounds of tests/team_solver_cases.py.  Wave mechanics: counts that leave a wave part-filled, easy and hard matrices
side by side (teams of one wave diverge), masked-off teams, and a few thousand matrices per variant compared bit for bit."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from tests import oracle_lib as ol
from tests import team_solver_cases as tc

pytestmark = pytest.mark.gpu

SENTINEL = -0.0078125   # what the records hold before a call: untouched records must still hold it


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def run_eig(variant, mats, active=None):
    mats = np.ascontiguousarray(np.stack(mats), dtype=np.float64)
    count, n = mats.shape[0], mats.shape[1]
    act = np.ones(count, dtype=np.int32) if active is None else np.ascontiguousarray(active, dtype=np.int32)
    rec = 1 + 2 * n + 2 * n * n
    team = np.full((count, rec), SENTINEL); single = np.full((count, rec), SENTINEL)
    capi.check(capi.lib().theia_hip_selftest_eig_team(variant, n, count, capi.ptr(mats, capi.C.c_double),
                                                      capi.ptr(act, capi.C.c_int32), capi.ptr(team, capi.C.c_double),
                                                      capi.ptr(single, capi.C.c_double)))
    return team, single


def unpack(r, n):
    return (r[0], r[1:1 + n], r[1 + n:1 + 2 * n], r[1 + 2 * n:1 + 2 * n + n * n].reshape(n, n),
            r[1 + 2 * n + n * n:].reshape(n, n))


def assert_eig_records_equal(variant, n, t, s, what, vectors=True):
    """team == one-thread bit for bit: ok, and for a success wr, wi, H and V (variant 2: the kept rows).  vectors=False: not
    V (non-finite input of n <= 2, which "succeeds" with NaN eigenvalues: a column whose wi is NaN is back-substituted by
    neither branch, and the back-transformation then reads the Schur form in the one-thread routine, zeros in the team's
    separate X -- DESIGN.md, stated deviations)."""
    ok_t, wr_t, wi_t, H_t, V_t = unpack(t, n)
    ok_s, wr_s, wi_s, H_s, V_s = unpack(s, n)
    assert ok_s in (0.0, 1.0), f"{what}: the one-thread runs with and without vectors disagree"
    assert ok_t == ok_s, f"{what}: ok team {ok_t} one-thread {ok_s}"
    if not ok_s:
        return
    assert np.array_equal(_bits(wr_t), _bits(wr_s)), f"{what}: wr"
    assert np.array_equal(_bits(wi_t), _bits(wi_s)), f"{what}: wi"
    assert np.array_equal(_bits(H_t), _bits(H_s)), f"{what}: Schur form"
    if not vectors:
        return
    if variant == 2:
        assert np.array_equal(_bits(V_t[:4]), _bits(V_s[tc.KEPT_ROWS])), f"{what}: kept rows of V"
        assert np.all(V_t[4:] == SENTINEL), f"{what}: the team wrote past its kept rows"
    else:
        assert np.array_equal(_bits(V_t), _bits(V_s)), f"{what}: V"


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_eig_team_families_bits_oracle_and_accuracy(variant):
    cplx = tc.VARIANT_CPLX[variant]
    worst, compared = 0.0, 0
    for n in tc.VARIANT_N[variant]:
        fams = tc.EIG_FAMILIES
        mats = [tc.eig_matrix(f, n) for f in fams]
        team, single = run_eig(variant, mats)
        for i, f in enumerate(fams):
            what = f"variant {variant} {f} n={n}"
            assert_eig_records_equal(variant, n, team[i], single[i], what, vectors=f not in tc.NONFINITE)
            compared += 1
            ok, wr, wi, H, V = unpack(single[i], n)
            ook, owr, owi, oH, oV = tc.eig_oracle(mats[i], cplx)
            assert bool(ok) == ook, what
            if f in tc.NONFINITE:
                assert not ook if n >= 3 else not (np.all(np.isfinite(owr)) and np.all(np.isfinite(owi))), what
                continue
            assert ook, what
            for a, b, name in ((wr, owr, "wr"), (wi, owi, "wi"), (H, oH, "H"), (V, oV, "V")):
                assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name} differs from the oracle"
            if n in tc.REF_N:
                worst = max(worst, tc.eig_accuracy(mats[i], wr, wi, V, cplx, tc.eig_reference(f, n), f in tc.DEFECTIVE))
    assert worst <= 1.0, worst
    print(f"\neig variant {variant}: {compared} matrices bit-identical to the one-thread routine and the oracle; "
          f"largest error / mpmath bound {worst:.3g}")


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_eig_team_action_matrices(variant):
    cplx = tc.VARIANT_CPLX[variant]
    worst = 0.0
    for kind in tc.VARIANT_ACTIONS[variant]:
        n = tc.ACTION_N[kind]
        mats = tc.action_matrices(kind, 24)
        team, single = run_eig(variant, mats)
        for i in range(len(mats)):
            what = f"variant {variant} {kind} #{i}"
            assert_eig_records_equal(variant, n, team[i], single[i], what)
            ok, wr, wi, H, V = unpack(single[i], n)
            ook, owr, owi, oH, oV = tc.eig_oracle(mats[i], cplx)
            assert ok == 1.0 and ook, what
            for a, b, name in ((wr, owr, "wr"), (wi, owi, "wi"), (H, oH, "H"), (V, oV, "V")):
                assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name} differs from the oracle"
        ok, wr, wi, H, V = unpack(single[0], n)
        worst = max(worst, tc.eig_accuracy(mats[0], wr, wi, V, cplx, tc.eig_reference(("action", kind, 0), None), False))
    assert worst <= 1.0, worst
    print(f"\neig variant {variant} action matrices: largest error / mpmath bound {worst:.3g}")


def _mixed(variant, count):
    """Easy and hard matrices alternating inside each wave: diagonal next to cyclic, zero next to Gaussian, identity next to
    a production action matrix."""
    n = {0: 10, 1: 13, 2: 27}[variant]
    act = tc.action_matrices(tc.VARIANT_ACTIONS[variant][-1], 8)
    pairs = [("diag_unsorted", "cyclic"), ("zero", "gauss"), ("identity", None), ("jordan", "rot_blocks")]
    out = []
    for i in range(count):
        easy, hard = pairs[(i // 2) % len(pairs)]
        if i % 2 == 0:
            out.append(tc.eig_matrix(easy, n))
        else:
            out.append(act[i % len(act)] if hard is None else tc.eig_matrix(hard, n))
    return out


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("count", [1, 7, 9, 13, 65])
def test_eig_team_partial_waves_divergence_and_masks(variant, count):
    mats = _mixed(variant, count)
    n = mats[0].shape[0]
    team, single = run_eig(variant, mats)
    for i in range(count):
        assert_eig_records_equal(variant, n, team[i], single[i], f"variant {variant} count {count} #{i}")
    # masked-off teams (holes, a masked first and last matrix): their records are untouched, the others unchanged
    active = np.array([(i % 3 != 1) and i != count - 1 for i in range(count)], dtype=np.int32)
    team2, single2 = run_eig(variant, mats, active)
    for i in range(count):
        if active[i]:
            assert np.array_equal(_bits(team2[i]), _bits(team[i])), f"#{i}: a masked neighbour changed the result"
            assert np.array_equal(_bits(single2[i]), _bits(single[i]))
        else:
            assert np.all(team2[i] == SENTINEL) and np.all(single2[i] == SENTINEL), f"#{i}: a masked record was written"


@pytest.mark.parametrize("variant,n", [(0, 10), (1, 8), (1, 13), (2, 27)])
def test_eig_team_soak_bits(variant, n):
    """About 4096 matrices per variant (Gaussian and production action matrices), team against one-thread bit for bit."""
    total = 2048 if (variant == 1) else 4096
    kinds = [k for k in tc.VARIANT_ACTIONS[variant] if tc.ACTION_N[k] == n]
    nact = total // 2
    acts = []
    for k in kinds:
        acts += tc.action_matrices(k, nact // len(kinds), seed=7)
    rng = np.random.default_rng(1000 + 10 * variant + n)
    mats = acts + [rng.normal(size=(n, n)) * 10.0 ** rng.integers(-3, 4) for _ in range(total - len(acts))]
    order = rng.permutation(len(mats))
    mats = [mats[i] for i in order]
    team, single = run_eig(variant, mats)
    bad = 0
    for i in range(len(mats)):
        try:
            assert_eig_records_equal(variant, n, team[i], single[i], f"#{i}")
        except AssertionError:
            bad += 1
    assert bad == 0, f"{bad} of {len(mats)} matrices differ"
    assert np.mean(single[:, 0] == 1.0) > 0.99
    print(f"\neig variant {variant} n={n}: {len(mats)} matrices bit-identical")


def run_svd(team_size, with_v, mats):
    mats = np.ascontiguousarray(np.stack(mats), dtype=np.float64)
    count = mats.shape[0]
    t = np.full((count, 171), SENTINEL); s = np.full((count, 171), SENTINEL)
    capi.check(capi.lib().theia_hip_selftest_svd9_team(team_size, with_v, count, capi.ptr(mats, capi.C.c_double),
                                                       capi.ptr(t, capi.C.c_double), capi.ptr(s, capi.C.c_double)))
    return t, s


@pytest.mark.parametrize("with_v", [0, 1])
@pytest.mark.parametrize("team_size", [5, 9])
def test_svd9_team_families(team_size, with_v):
    mats = [tc.svd_matrix(f) for f in tc.SVD_FAMILIES]
    rng = np.random.default_rng(team_size * 2 + with_v)
    extra = [rng.normal(size=(9, 9)) if i % 2 else tc.svd_matrix("omega") * rng.uniform(0.5, 2) for i in range(4096 - len(mats))]
    t, s = run_svd(team_size, with_v, mats + extra)
    width = 171 if with_v else 90
    diff = np.nonzero(np.any(_bits(t[:, :width]) != _bits(s[:, :width]), axis=1))[0]
    assert len(diff) == 0, f"{len(diff)} matrices differ, first {diff[:5]}"
    if not with_v:
        assert np.all(t[:, 90:] == SENTINEL)
    worst = 0.0
    for i, f in enumerate(tc.SVD_FAMILIES):
        Uo, So, Vo = ol.svd9(mats[i])
        assert np.array_equal(_bits(s[i, :81]), _bits(Uo.ravel())) and np.array_equal(_bits(s[i, 81:90]), _bits(So))
        assert np.array_equal(_bits(s[i, 90:]), _bits(Vo.ravel())), f
        worst = max(worst, tc.svd_accuracy(mats[i], s[i, :81].reshape(9, 9), s[i, 81:90], s[i, 90:].reshape(9, 9),
                                           tc.svd_reference(f)))
    assert worst <= 1.0, worst
    print(f"\nsvd9_team<{team_size}> with_v={with_v}: {len(t)} matrices bit-identical; largest error / mpmath bound {worst:.3g}")


@pytest.mark.parametrize("count", [1, 11, 12, 13, 65])
def test_svd9_team_partial_waves(count):
    mats = [tc.svd_matrix(tc.SVD_FAMILIES[i % len(tc.SVD_FAMILIES)]) for i in range(count)]
    for team_size in (5, 9):
        t, s = run_svd(team_size, 1, mats)
        assert np.array_equal(_bits(t), _bits(s)), (team_size, count)


def run_fp(corrs):
    corr = np.ascontiguousarray(np.stack(corrs), dtype=np.float64)
    count = corr.shape[0]
    t = np.full((count, 137), SENTINEL); s = np.full((count, 137), SENTINEL)
    capi.check(capi.lib().theia_hip_selftest_five_point_pre_team(count, capi.ptr(corr, capi.C.c_double),
                                                                 capi.ptr(t, capi.C.c_double), capi.ptr(s, capi.C.c_double)))
    return t, s


def test_five_point_pre_team_families():
    corrs, names = [], []
    for f in tc.FP_FAMILIES:
        for seed in range(8):
            corrs.append(tc.fp_corr(f, seed)); names.append(f"{f}/{seed}")
    t, s = run_fp(corrs)
    worst, nok = 0.0, 0
    for i, c in enumerate(corrs):
        assert t[i, 0] == s[i, 0], names[i]
        ook, N, M = tc.five_point_pre_oracle(c)
        assert bool(s[i, 0]) == ook == (tc.exact_rank(tc.fp_system(c)) == 5), names[i]
        if ook:
            nok += 1
            assert np.array_equal(_bits(t[i]), _bits(s[i])), names[i]
            assert np.array_equal(_bits(s[i, 1:37]), _bits(N.ravel())) and np.array_equal(_bits(s[i, 37:]), _bits(M.ravel())), names[i]
            worst = max(worst, tc.fp_null_ratio(c, N))
        else:
            assert np.all(t[i, 1:] == SENTINEL) and np.all(s[i, 1:] == SENTINEL), names[i]
    assert worst <= 1.0 and nok >= 16
    print(f"\nfive_point_pre_team: {len(corrs)} problems, {nok} of rank 5; largest |Q N| / bound {worst:.3g}")


def test_five_point_pre_team_soak_bits():
    rng = np.random.default_rng(55)
    corrs = []
    for i in range(4096):
        if i % 4 == 0:
            corrs.append(rng.integers(-3, 4, size=(5, 4)).astype(np.float64))   # pivot ties
        else:
            corrs.append(rng.normal(size=(5, 4)) * 10.0 ** rng.integers(-2, 2))
    t, s = run_fp(corrs)
    assert np.array_equal(t[:, 0], s[:, 0])
    ok = s[:, 0] == 1.0
    assert np.array_equal(_bits(t[ok]), _bits(s[ok]))
    assert np.all(t[~ok, 1:] == SENTINEL)
    assert ok.mean() > 0.7
    print(f"\nfive_point_pre_team: {len(corrs)} problems bit-identical ({int(ok.sum())} of rank 5)")


def test_selftest_entries_refuse_bad_arguments():
    L = capi.lib()
    A = np.zeros((1, 27, 27)); act = np.ones(1, dtype=np.int32); o1 = np.zeros(2000); o2 = np.zeros(2000)
    dp = lambda a: capi.ptr(a, capi.C.c_double)   # noqa: E731
    ip = capi.ptr(act, capi.C.c_int32)
    E = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    for variant, n in ((3, 10), (-1, 10), (0, 0), (0, 11), (1, 14), (2, 9), (2, 28)):
        assert L.theia_hip_selftest_eig_team(variant, n, 1, dp(A), ip, dp(o1), dp(o2)) == E, (variant, n)
    assert L.theia_hip_selftest_eig_team(0, 10, 0, dp(A), ip, dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_eig_team(0, 10, 1, None, ip, dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_eig_team(0, 10, 1, dp(A), None, dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_eig_team(0, 10, 1, dp(A), ip, None, dp(o2)) == E
    assert L.theia_hip_selftest_eig_team(0, 10, 1, dp(A), ip, dp(o1), None) == E
    for team_size, with_v in ((4, 0), (16, 1), (5, 2)):
        assert L.theia_hip_selftest_svd9_team(team_size, with_v, 1, dp(A), dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_svd9_team(5, 0, 0, dp(A), dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_svd9_team(5, 0, 1, None, dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_five_point_pre_team(0, dp(A), dp(o1), dp(o2)) == E
    assert L.theia_hip_selftest_five_point_pre_team(1, dp(A), None, dp(o2)) == E
