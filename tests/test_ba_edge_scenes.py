"""CPU: the edge scenes of tests/ba_edge_scenes.py are what the GPU instance matrix (test_ba_instances_gpu.py) takes them
for.  Every branch condition is restated in numpy on the start state and must be taken by at least three observations; the
oracle must be valid and finite on every scene, loss and point parametrisation; the robust cases must leave every block
enough observations with a nonzero weight for a trajectory comparison to mean something; the two invalid-observation
scenes must have the property their GPU tests rely on.  These are conditions on the scenes, checked with the oracle alone."""
import numpy as np
import pytest

from tests import ba_edge_scenes as es
from tests import oracle_lib as ol

MODELS = list(range(8))
# the branches every scene must take, and those of one model
COMMON = ["rotation_small", "rotation_exact_zero", "rotation_rodrigues", "householder_sigma_small", "householder_w_positive", "w_quarter"]
PER_MODEL = {
    2: ["fisheye_on_axis", "fisheye_behind", "fisheye_general"],
    3: ["fov_small_omega", "fov_small_radius", "fov_general"],
    4: ["division_denominator_zero", "division_inner_negative", "division_general"],
    5: ["ds_alpha_le_half", "ds_alpha_gt_half"],
    6: ["eucm_alpha_le_half", "eucm_alpha_gt_half"],
}


@pytest.mark.parametrize("model", MODELS)
def test_every_branch_is_taken_by_three_observations(model):
    p = es.edge_scene(model)
    counts = es.branch_counts(p)
    print(model, counts)
    want = COMMON + PER_MODEL.get(model, []) + (["householder_w_nonpositive"] if model in es.NEGATIVE_W_MODELS else [])
    for name in want:
        assert counts[name] >= 3, (model, name, counts[name])
    assert counts["invalid"] == 0
    if model == 4:   # the sqrt(1 - 4 k ru^2) of the general branch stays away from its singularity
        assert counts["division_min_general_inner"] > 0.25


@pytest.mark.parametrize("model", MODELS)
def test_scene_shape(model):
    p = es.edge_scene(model)
    lengths = np.bincount(p.obs_pt)
    assert p.cam_ext.shape[0] == 12 and 200 <= p.points.shape[0] <= 220 and p.intrinsics.shape[0] == 3
    assert lengths.min() == 2 and lengths.max() == 10 and set(range(2, 11)) <= set(lengths.tolist())
    assert set(p.cam_group[p.obs_cam].tolist()) == {0, 1, 2}
    # cameras 0 and 1 share tracks nobody else sees
    only01 = [t for t in range(p.points.shape[0]) if set(p.obs_cam[p.obs_pt == t].tolist()) == {0, 1}]
    assert len(only01) >= 10
    # the same scene twice: the same bits
    q = es._edge_scene.__wrapped__((model,) * 3, 1, 1.0, model in es.NEGATIVE_W_MODELS)[0]
    assert np.array_equal(q.obs_uv, p.obs_uv) and np.array_equal(q.points, p.points) and np.array_equal(q.cam_ext, p.cam_ext)


@pytest.mark.parametrize("model", MODELS)
def test_oracle_is_valid_and_finite_on_every_case(model):
    for loss in es.LOSSES:
        p = es.case_scene(model, loss)
        for pd in (3, 4):
            o = es.set_case(ol.default_options(), loss, pd)
            ok, cost, r, jc, jp = ol.evaluate(p, o)
            assert ok == 1 and np.isfinite(cost) and np.isfinite(r).all() and np.isfinite(jc).all() and np.isfinite(jp).all(), (loss, pd)
            S, rhs = ol.reduced_system(p, o, 1e4)
            assert S.shape == (72, 72) and np.isfinite(S).all() and np.isfinite(rhs).all(), (loss, pd)


@pytest.mark.parametrize("model", MODELS)
def test_robust_cases_keep_their_observations(model):
    """Tukey and Truncated: at most a quarter of the observations with rho' == 0, and every camera and every point keeps at
    least two observations with a nonzero weight (no block is left to the LM diagonal alone)."""
    for loss in (5, 6):
        p = es.case_scene(model, loss)
        _, _, r, _, _ = ol.evaluate(p, es.set_case(ol.default_options(), 0, 3))   # the unweighted residuals
        zero = es.zero_weight(loss, es.LOSS_WIDTH[loss], r)
        # the restated condition against the oracle's own loss: rho' of the weighted residual is sqrt(rho') r
        _, _, rw, _, _ = ol.evaluate(p, es.set_case(ol.default_options(), loss, 3))
        assert np.array_equal(zero, ((rw ** 2).sum(1) == 0.0) & ((r ** 2).sum(1) > 0.0))
        print(model, es.LOSS_NAMES[loss], "zero weight: %d of %d" % (zero.sum(), len(zero)))
        assert zero.mean() <= 0.25
        assert np.bincount(p.obs_cam[~zero], minlength=p.cam_ext.shape[0]).min() >= 2
        assert np.bincount(p.obs_pt[~zero], minlength=p.points.shape[0]).min() >= 2


def test_long_track_scene():
    p = es.with_long_tracks(es.edge_scene(0))
    lengths = np.bincount(p.obs_pt)
    assert (lengths == 65).sum() == 2 and lengths.max() == 65
    assert ol.evaluate(p, ol.default_options())[0] == 1


def test_invalid_start_scene_is_invalid_in_the_oracle():
    p = es.invalid_start_scene()
    assert es.branch_counts(p)["invalid"] >= 1
    for intr in (0, 0x11):
        o = es.set_case(ol.default_options(), 0, 3, intrinsics_to_optimize=intr)
        assert ol.evaluate(p, o)[0] == 0
        q = p.copy()
        s, tr = ol.solve(q, o)
        assert s.success == 0 and s.num_iterations == 0
        assert np.array_equal(q.cam_ext, p.cam_ext) and np.array_equal(q.points, p.points) and np.array_equal(q.intrinsics, p.intrinsics)


@pytest.mark.parametrize("intr", [0, 0x11])
@pytest.mark.parametrize("pd", [3, 4])
def test_invalid_candidate_scene_rejects_its_first_step(pd, intr):
    p, idx, target = es.invalid_candidate_scene()
    assert es.branch_counts(p)["invalid"] == 0          # valid at the start ...
    q = p.copy(); q.points[idx, :3] = target
    sel = (q.obs_pt == idx) & (q.obs_cam == 6)
    valid = es.model_valid(es.INVALID_MODEL, q.intrinsics[q.cam_group[q.obs_cam]], es.camera_frame(q.cam_ext, q.points, q.obs_cam, q.obs_pt))
    assert sel.sum() == 1 and not valid[sel][0] and valid[~sel].all()   # ... and invalid, in camera 6 alone, where the others pull the point
    o = es.set_case(ol.default_options(), 0, pd, intrinsics_to_optimize=intr, max_num_iterations=8)
    assert ol.evaluate(p, o)[0] == 1
    po = p.copy()
    s, tr = ol.solve(po, o)
    acc = tr.accepted[: tr.size].tolist()
    print(pd, intr, acc, tr.cost[: tr.size].tolist())
    assert acc[0] == 1 and acc[1] == 0 and tr.cost[1] > 1e300      # the first candidate fails to evaluate: rejected
    assert 1 in acc[2:]                                          # and a later, shorter step is taken
    assert es.branch_counts(po)["invalid"] == 0
