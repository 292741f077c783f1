"""GPU: theia_hip_lud_positions against the numpy restatement (tests/lud_positions_ref.py), the pyTheia-named mirror,
the device-side stopping test under an iteration cap, and the C-ABI's refusals."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from tests import lud_positions_ref as ref
from tests import position_scenes as ps

pytestmark = pytest.mark.gpu

# name: (views, pairs, noise in degrees, outlier fraction, held views, duplicate / reversed pairs, seed,
#        tolerance after alignment or None)
CASES = {
    "SmallTestNoNoise": (4, 6, 0.0, 0.0, 1, 0, 0, 1e-2),
    "SmallTestWithNoise": (4, 6, 1.0, 0.0, 1, 0, 0, 0.1),
    "TestNoNoise": (200, 500, 0.0, 0.0, 1, 0, 0, 0.5),
    "TestWithNoise": (200, 500, 1.0, 0.0, 1, 0, 0, 1.0),
    "v100_outliers": (100, 800, 2.0, 0.1, 1, 0, 1, None),
    "v60_duplicate_reversed": (60, 400, 2.0, 0.1, 1, 20, 2, None),
    "v80_three_held": (80, 500, 2.0, 0.0, 3, 0, 3, None),
    "m21": (22, 90, 2.0, 0.0, 1, 0, 4, None),
    "m22": (23, 90, 2.0, 0.0, 1, 0, 5, None),
    "m64": (65, 300, 2.0, 0.1, 1, 0, 6, None),
    "m65": (66, 300, 2.0, 0.1, 1, 0, 7, None),
    "v2000_outliers": (2000, 30000, 2.0, 0.1, 1, 0, 1, None),
}


def _scene(name):
    n, pairs, noise, out, nheld, dup, seed, tol = CASES[name]
    s = ps.make_scene(n, pairs, noise, out, seed=seed)
    if dup:
        s = ps.with_duplicates(s, dup, dup, seed=seed)
    return s, np.arange(n) < nheld, tol


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(name):
    s, fixed, tol = _scene(name)
    form = "schur" if s["n"] > 500 else "full"   # the same system (test_lud_positions.py), a dense solve at 2 000 views
    r = ref.lud_positions(s["orientations"], s["edges"], s["rel"], fixed, form=form)
    rc, got, summ = global_pose.lud_positions(s["orientations"], s["edges"], s["rel"], fixed)
    assert rc == 0, capi.lib().theia_hip_last_error()
    # equal iteration counts only mean something when no convergence decision of the restatement is a near tie
    assert min(r["margins"]) > 1e-6
    assert summ.admm_iterations == r["admm_iterations"]
    assert bool(summ.converged) == r["converged"]
    ext = ps.extent(r["positions"])
    assert np.abs(got - r["positions"]).max() <= 1e-8 * ext
    for k in ("r_norm", "s_norm", "primal_eps", "dual_eps"):
        assert abs(getattr(summ, k) - r[k]) <= 1e-6 * max(abs(r[k]), 1e-12), k
    assert np.all(got[fixed] == 0.0)
    if tol is not None:
        assert ps.aligned_errors(got, s["gt"]).max() < tol
    rc2, again, summ2 = global_pose.lud_positions(s["orientations"], s["edges"], s["rel"], fixed)
    assert rc2 == 0 and np.array_equal(again, got)   # bit-identical
    assert summ2.admm_iterations == summ.admm_iterations and summ2.r_norm == summ.r_norm and summ2.s_norm == summ.s_norm


@pytest.mark.parametrize("name", ["SmallTestNoNoise", "v100_outliers"])
def test_iteration_cap_and_converged_flag(name):
    s, fixed, _ = _scene(name)
    for cap in (1, 3, 33):
        o = global_pose.ConstrainedL1SolverOptions()
        o.max_num_iterations = cap
        r = ref.lud_positions(s["orientations"], s["edges"], s["rel"], fixed, ref.SolverOptions(max_num_iterations=cap))
        rc, got, summ = global_pose.lud_positions(s["orientations"], s["edges"], s["rel"], fixed, o)
        assert rc == 0
        assert summ.admm_iterations == r["admm_iterations"] <= cap
        assert bool(summ.converged) == r["converged"]
        if summ.admm_iterations == cap:
            assert bool(summ.converged) == (summ.r_norm < summ.primal_eps and summ.s_norm < summ.dual_eps)
        assert np.abs(got - r["positions"]).max() <= 1e-8 * ps.extent(r["positions"])
    # a run that converges stops at the restatement's iteration, well inside the cap, and reports it
    r = ref.lud_positions(s["orientations"], s["edges"], s["rel"], fixed)
    if r["converged"]:
        _, _, summ = global_pose.lud_positions(s["orientations"], s["edges"], s["rel"], fixed)
        assert summ.converged and summ.admm_iterations == r["admm_iterations"] < 1000


def test_mirror_api():
    """pyTheia's calling sequence: {(id1, id2): TwoViewInfo} and {id: orientation} in, {id: position} out; views of
    pairs without an orientation are refused, views without a pair get no entry; the first view is held."""
    from pytheiasfm_amd.twoview import TwoViewInfo
    s = ps.make_scene(30, 150, 1.0, seed=4)
    ids = [10 * i + 3 for i in range(30)]
    pairs = {}
    for (a, b), t in zip(s["edges"], s["rel"]):
        info = TwoViewInfo(); info.position_2 = t.copy()
        pairs[(ids[a], ids[b])] = info
    orient = {ids[i]: s["orientations"][i].copy() for i in range(30)}
    orient[999] = np.zeros(3)   # a view with no pair: no entry in the output
    est = sfm.LeastUnsquaredDeviationPositionEstimator(sfm.LeastUnsquaredDeviationPositionEstimatorOptions())
    out = est.EstimatePositions(pairs, orient)
    assert sorted(out) == sorted(ids) and 999 not in out
    r = ref.lud_positions(s["orientations"], s["edges"], s["rel"])
    got = np.array([out[v] for v in ids])
    assert np.abs(got - r["positions"]).max() <= 1e-8 * ps.extent(r["positions"])
    assert est.last_summary.admm_iterations == r["admm_iterations"]
    assert ps.aligned_errors(got, s["gt"]).max() < 0.5
    # a pair whose first view in the dict is another one: the positions move by a translation only
    first = (ids[5], ids[6])
    pairs2 = {first: pairs[first]}
    pairs2.update({k: v for k, v in pairs.items() if k != first})
    out2 = est.EstimatePositions(pairs2, orient)
    assert np.all(out2[ids[5]] == 0.0)
    got2 = np.array([out2[v] for v in ids])
    if est.last_summary.admm_iterations == r["admm_iterations"]:
        assert np.abs(got2 - (got - got[5])).max() <= 1e-6 * ps.extent(got)


def test_refusals_leave_the_positions_untouched():
    s = ps.make_scene(20, 60, 2.0, seed=9)
    aa, e, t = s["orientations"], s["edges"], s["rel"]
    two = np.concatenate([aa, np.zeros((2, 3))])
    one = [[1.0, 0.0, 0.0]]
    cases = [(two, np.concatenate([e, [[20, 21]]]), np.concatenate([t, one]), None, None),       # component without a held view
             (two, e, t, None, None),                                                             # isolated free views
             (aa, np.concatenate([e, [[3, 20]]]), np.concatenate([t, one]), None, None),         # edge out of range
             (aa, np.concatenate([e, [[-1, 2]]]), np.concatenate([t, one]), None, None),         # negative index
             (aa, e[:0], t[:0], None, None),                                                      # no pairs
             (aa, e, t, None, dict(max_num_iterations=0)), (aa, e, t, None, dict(max_num_iterations=-5)),
             (aa, e, t, None, dict(rho=0.0)), (aa, e, t, None, dict(rho=-10.0))]
    for orient, edges, rel, fixed, bad in cases:
        o = global_pose.ConstrainedL1SolverOptions()
        for k, v in (bad or {}).items():
            setattr(o, k, v)
        out = np.full((orient.shape[0], 3), -3.5)
        rc, got, _ = global_pose.lud_positions(orient, edges, rel, fixed, o, positions_out=out)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
        assert np.all(out == -3.5)
    # holding a view of the second component makes the same graph solvable
    f = np.zeros(22, dtype=bool); f[0] = True; f[20] = True
    rc, got, _ = global_pose.lud_positions(two, np.concatenate([e, [[20, 21]]]), np.concatenate([t, one]), f)
    assert rc == 0 and np.all(got[20] == 0.0) and np.all(got[0] == 0.0)
    # the device still works after the refusals
    rc, got, summ = global_pose.lud_positions(aa, e, t)
    assert rc == 0 and summ.admm_iterations >= 1
