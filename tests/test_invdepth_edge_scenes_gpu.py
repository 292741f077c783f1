"""GPU: the inverse-depth path (csrc/ba_invdepth.hip: id_observe with its c == cr branch, k_id_track's per-track rank-one
Schur elimination, back-substitution, LM driver) against the oracle's dense Jet-based LM on the cases of
tests/invdepth_edge_scenes.py: all eight camera models x four option sets, the remaining losses, a mixed-model scene, the
first LM step of each alone ("@1"), the structures of k_id_track (reference view last / highest / not an observer,
constant and partly frozen cameras on either side, constant tracks, n == 0, tracks seen by every camera, sqrt information,
eight of nine variable groups and the refusal at nine), two banded scenes on the tile-sparse and the dense plan, and the
handle path.  The tolerances are those of test_invdepth_gpu.py (tests/invdepth.compare); every case was admitted by
test_invdepth_edge_scenes.py with the oracle alone at a tenth of them.

The rho of a reference-only track is unobservable in a central model (round-off amplified by the LM step; the oracle's own
moves between two runs): it is left out of the rho comparison for every model but the orthographic one, and must be finite
and positive; every other block is compared.  The step norm carries the same round-off and is compared where the scene
has no such track.

Measured on an MI355X (two runs, the same verdicts; every case prints its figures): the largest deviation of any case, in
units of its tolerance, was 0.49 (intrinsics, every camera constant with a free group), 0.31 / 0.23 / 0.23 for the intrinsics
of the models 6 / 5 / 2, 0.017 for a cost, 0.012 for a gradient, 7e-4 for a camera (7e-12 absolute), 5e-3 for a rho, 0.011 for a step norm.  Two
deliberately wrong builds, for the record: the Schur term of add_pair transposed for one order of the two offsets fails 203
of these tests; the tile plan built without the slots of the reference camera passes every test of test_invdepth_gpu.py
and fails the six arc34far ones."""
import functools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba
from tests import invdepth as idp
from tests import invdepth_edge_scenes as ies

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(name):
    case = ies.CASES[name]
    return ies.solve_oracle(case, case.problem())


def _device(case, p):
    q = p.copy()
    s, tr = ba.solve(q, case.set_options(ba.default_options()))
    return q, s, tr


def _check(name, g, o, p):
    """compare() plus what a solve must leave alone."""
    case = ies.CASES[name]
    skip = case.skip_rho(p)
    idp.compare(g, o, skip_rho=skip, step_norm=skip is None, label=name)
    q = g[0]
    if skip is not None:
        assert np.isfinite(q.point_inverse_depth[skip]).all() and (q.point_inverse_depth[skip] > 0.0).all(), q.point_inverse_depth[skip]
    assert np.array_equal(q.cam_ext[(p.cam_const & 1) != 0, :3], p.cam_ext[(p.cam_const & 1) != 0, :3])
    assert np.array_equal(q.cam_ext[(p.cam_const & 2) != 0, 3:], p.cam_ext[(p.cam_const & 2) != 0, 3:])
    if p.point_const is not None:
        fixed = p.point_const != 0
        assert np.array_equal(q.point_inverse_depth[fixed], p.point_inverse_depth[fixed])
    if not case.options.get("intrinsics_to_optimize", 0):
        assert np.array_equal(q.intrinsics, p.intrinsics)
    elif p.group_const is not None:
        assert np.array_equal(q.intrinsics[p.group_const != 0], p.intrinsics[p.group_const != 0])


@pytest.mark.parametrize("name", list(ies.CASES))
def test_case_follows_the_oracle(name):
    case = ies.CASES[name]
    p = case.problem()
    g, o = _device(case, p), _oracle(name)
    _check(name, g, o, p)
    if case.iters == 1:      # initial cost, first gradient, the step, the cost after it: two trace rows, nothing else
        assert g[2].size == 2 and o[2].size == 2 and g[1].num_iterations == 1


@pytest.mark.parametrize("name", ies.TILE_CASES)
def test_tile_scenes_on_both_plans(name, monkeypatch):
    """The banded scenes: reduced cameras (and, on the ring, group 0) straddle a 64-wide tile; on the arc the tiles 0 and 2 are
    not coupled, so the tile-sparse plan leaves that tile pair out -- or (arc34far) coupled by reference views that do not
    observe, and by nothing else.  The tile-sparse plan and the dense schedule of the same
    library both follow the oracle, and each other as in test_inverse_depth_tile_sparse_reduced_system."""
    case = ies.CASES[name]
    p = case.problem()
    h = ba.BaHandle(p.copy(), case.set_options(ba.default_options()))
    n = h.plan_info()["n"]
    h.close()
    assert n == ies.structure_counts(p, case.options.get("intrinsics_to_optimize", 0))["n"]     # the layout the CPU file restates
    g = _device(case, p)
    _check(name, g, _oracle(name), p)
    monkeypatch.setenv("THEIA_HIP_INVDEPTH_DENSE", "1")
    d = _device(case, p)
    _check(name, d, _oracle(name), p)
    assert d[1].num_iterations == g[1].num_iterations and np.allclose(d[2].cost, g[2].cost, rtol=1e-11)
    assert np.abs(d[0].cam_ext - g[0].cam_ext).max() <= 1e-9


@pytest.mark.parametrize("model", [0, 2])
def test_nine_variable_groups_are_refused(model):
    """One group more than k_id_track's table holds: THEIA_HIP_ERR_UNSUPPORTED, the parameters untouched (the same scene with
    the ninth group constant is the case eight-of-nine-groups-intr11)."""
    p = ies.nine_groups_scene(model, True)
    q = p.copy()
    o = ba.default_options(); o.max_num_iterations = 3; o.use_inner_iterations = 0; o.intrinsics_to_optimize = 0x11
    with pytest.raises(capi.TheiaHipError) as e:
        ba.solve(q, o)
    assert e.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED
    assert np.array_equal(q.cam_ext, p.cam_ext) and np.array_equal(q.intrinsics, p.intrinsics)
    assert np.array_equal(q.point_inverse_depth, p.point_inverse_depth)
    o.intrinsics_to_optimize = 0                      # no variable group: nothing to refuse
    s, _ = ba.solve(q, o)
    assert s.success


def test_handle_path_equals_the_one_shot_solve():
    """theia_hip_ba_create / run / download on a non-pinhole scene (fisheye model, free focal length and distortion)."""
    name = "model2-intr11-observable"
    case = ies.CASES[name]
    p = case.problem()
    one = _device(case, p)
    hp = p.copy()
    with ba.BaHandle(hp, case.set_options(ba.default_options())) as h:
        s, tr = h.run(); h.download(hp)
    _check(name, (hp, s, tr), _oracle(name), p)
    assert s.num_iterations == one[1].num_iterations and np.allclose(tr.cost, one[2].cost, rtol=1e-10)
    assert np.allclose(hp.cam_ext, one[0].cam_ext, rtol=1e-9, atol=1e-11) and np.allclose(hp.intrinsics, one[0].intrinsics, rtol=1e-9, atol=1e-12)
    assert np.allclose(hp.point_inverse_depth, one[0].point_inverse_depth, rtol=1e-9, atol=1e-12)
