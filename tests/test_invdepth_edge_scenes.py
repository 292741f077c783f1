"""CPU: the inverse-depth edge scenes of tests/invdepth_edge_scenes.py are what the GPU file
(test_invdepth_edge_scenes_gpu.py) takes them for.  Every structural branch of csrc/ba_invdepth.hip's k_id_obs / k_id_track
the scenes are built for is restated in numpy and must be taken; the camera-model branches of ba_edge_scenes.branch_counts
must survive the conversion; and every (scene, options, iterations) case is ADMITTED with the oracle alone: two runs on
inputs 1e-15 apart give the same accept list, agree in every compared quantity to a tenth of the tolerance the GPU test
uses, and the bound on the round-off walk of the reference-only tracks' unobservable rho (invdepth_edge_scenes.wander_bound)
leaves it positive."""
import numpy as np
import pytest

from tests import ba_edge_scenes as es
from tests import invdepth as idp
from tests import invdepth_edge_scenes as ies
from tests import oracle_lib as ol
from tests.test_ba_edge_scenes import PER_MODEL

MODELS = list(range(8))


# ---------------------------------------------------------------- the converter
@pytest.mark.parametrize("reference", ["first", "last", "highest", "non_observer"])
def test_converter_reproduces_the_points_and_picks_the_reference(reference):
    p = es.edge_scene(2, 1, negative_w=False)               # fisheye: points BEHIND cameras 5 and 8 must not become references
    q = idp.from_problem(p, reference)
    X = ies.as_points_problem(q).points
    assert np.abs(X[:, :3] - p.points[:, :3] / p.points[:, 3:4]).max() <= 1e-12       # b / rho is the start point
    depth = es.camera_frame(p.cam_ext, p.points, p.obs_cam, p.obs_pt)[:, 2] / p.points[p.obs_pt, 3]
    for t in range(p.points.shape[0]):
        sel = np.nonzero((p.obs_pt == t) & (depth > 0.5))[0]
        want = {"first": p.obs_cam[sel[0]], "non_observer": p.obs_cam[sel[0]], "last": p.obs_cam[sel[-1]], "highest": p.obs_cam[sel].max()}[reference]
        assert q.point_ref_cam[t] == want
    assert (q.point_inverse_depth > 0).all() and np.array_equal(q.point_ref_bearing[:, 2], np.ones(len(X)))
    seen_by_ref = np.bincount(q.obs_pt[q.obs_cam == q.point_ref_cam[q.obs_pt]], minlength=len(X))
    if reference == "non_observer":
        assert (seen_by_ref == 0).all() and len(q.obs_pt) == len(p.obs_pt) - len(X)
    else:
        assert (seen_by_ref == 1).all() and len(q.obs_pt) == len(p.obs_pt)
    assert (depth < 0).sum() >= 4                            # (the scene does have them)


def test_reference_only_helpers():
    q = idp.from_problem(es.edge_scene(0, 1, negative_w=False), "first")
    assert not idp.reference_only(q).any()
    cut = idp.cut_to_reference(q, [30, 40, 41])
    mask = idp.reference_only(cut)
    assert np.nonzero(mask)[0].tolist() == [30, 40, 41] and (np.bincount(cut.obs_pt)[mask] == 1).all()
    gone = idp.without_reference_observation(q, [50])
    assert len(gone.obs_pt) == len(q.obs_pt) - 1 and not idp.reference_only(gone).any()
    assert not ((gone.obs_pt == 50) & (gone.obs_cam == gone.point_ref_cam[50])).any()


# ---------------------------------------------------------------- branch counts
@pytest.mark.parametrize("model", MODELS)
def test_model_scene_takes_the_structural_branches(model):
    p = ies.model_scene(model)
    for mask in (0, 0x11):
        c = ies.structure_counts(p, mask)
        print(model, hex(mask), c)
        assert c["reference_only_tracks"] == 10 and c["tracks_without_reference_observation"] == 10
        for name in ("obs_in_reference_view", "const_ref_variable_observer", "variable_ref_const_observer", "partly_frozen_ref",
                     "partly_frozen_observer", "observer_above_ref", "observer_below_ref", "later_observer_above", "later_observer_below"):
            assert c[name] >= 3, (name, c[name])
        assert c["ncam6"] == 60 and c["n"] == (60 if mask == 0 else 90)
    assert c["track_groups"][1] >= 3 and c["track_groups"][2] >= 3 and c["track_groups"][3] >= 3     # 1, 2 and 3 variable groups
    assert not idp.reference_only(ies.model_scene(model, ref_only=False)).any()


@pytest.mark.parametrize("model", MODELS)
def test_model_scene_keeps_the_camera_model_branches(model):
    """ba_edge_scenes.branch_counts on the world points of the converted scene (X = R_ref^T b / rho + c_ref)."""
    counts = es.branch_counts(ies.as_points_problem(ies.model_scene(model)))
    print(model, counts)
    for name in ["rotation_small", "rotation_exact_zero", "rotation_rodrigues"] + PER_MODEL.get(model, []):
        assert counts[name] >= 3, (name, counts[name])
    assert counts["invalid"] == 0


@pytest.mark.parametrize("model", [0, 2])
def test_structure_scenes(model):
    c = ies.structure_counts(ies.model_scene(model, reference="highest", ref_only=False), 0x11)
    assert c["observer_below_ref"] == 0 or c["observer_above_ref"] > 5 * c["observer_below_ref"]    # the reference block lies below
    c = ies.structure_counts(ies.model_scene(model, reference="non_observer", ref_only=False), 0x11)
    assert c["obs_in_reference_view"] == 0 and c["tracks_without_reference_observation"] >= 200
    c = ies.structure_counts(ies.frozen_scene(model), 0x11)
    for name in ("const_ref_variable_observer", "variable_ref_const_observer", "partly_frozen_ref", "partly_frozen_observer"):
        assert c[name] >= 10, (name, c[name])
    c = ies.structure_counts(ies.constant_tracks_scene(model), 0)
    assert c["constant_tracks"] >= 30
    for mask, n in ((0, 0), (0x11, 30)):
        c = ies.structure_counts(ies.all_cameras_constant_scene(model), mask)
        assert c["ncam6"] == 0 and c["n"] == n
    c = ies.structure_counts(ies.full_tracks_scene(model), 0x11)
    assert c["tracks_seen_by_all"] == 3
    p = ies.sqrt_info_scene(model)
    assert p.obs_sqrt_info.min() >= 0.5 and p.obs_sqrt_info.max() <= 2.0 and np.abs(p.obs_sqrt_info - 1.0).min() > 1e-6
    c = ies.structure_counts(ies.nine_groups_scene(model, False), 0x11)
    print(model, "nine groups", c["track_groups"])
    assert c["track_groups"][8] >= 1 and c["track_groups"][9:].sum() == 0 and c["track_groups"][2] >= 1 and c["track_groups"][3] >= 1
    c = ies.structure_counts(ies.nine_groups_scene(model, True), 0x11)
    assert c["track_groups"][9] >= 1                                                                  # one group more than the table holds


def test_tile_scenes():
    p = ies.ring22_scene()
    c = ies.structure_counts(p, 0)
    assert c["ncam6"] == 120 and c["n"] == 120 and c["tiles"] == 2 and c["cameras_straddling_a_tile"] == [12]     # reduced camera 10: slots 60 .. 65
    c = ies.structure_counts(p, 0x11)
    assert c["n"] == 140 and c["tiles"] == 3 and c["cameras_straddling_a_tile"] == [12] and c["groups_straddling_a_tile"] == [0]   # slots 120 .. 129
    cam_red = ies.reduced_layout(p, 0)[0]
    # the camera tiles 0 and 1 meet only in tracks of the band around the boundary and where the ring closes
    for t in np.unique(p.obs_pt):
        cams = [c_ for c_ in set(p.obs_cam[p.obs_pt == t].tolist()) if cam_red[c_] >= 0]
        tiles = {s for c_ in cams for s in ies._tiles(6 * cam_red[c_], 6)}
        if tiles == {0, 1}:
            assert set(cams) & {9, 10, 11, 12, 13, 14, 15, 21, 2, 3, 4}
    p = ies.arc34_scene()
    c = ies.structure_counts(p, 0)
    assert c["ncam6"] == 192 and c["tiles"] == 3 and c["cameras_straddling_a_tile"] == [12, 23] and c["uncoupled_tile_pairs"] == 1
    adj = ies.tile_adjacency(p, 0)
    assert adj[0, 1] and adj[1, 2] and not adj[0, 2]
    c = ies.structure_counts(p, 0x11)
    assert c["n"] == 212 and c["tiles"] == 4 and c["uncoupled_tile_pairs"] == 1 and not ies.tile_adjacency(p, 0x11)[0, 2]
    # the same arc with six tracks whose reference view (tile 0) does not observe and whose observers are in tile 2
    q = ies.arc34_far_reference_scene()
    adj = ies.tile_adjacency(q, 0)
    assert adj[0, 2] and ies.structure_counts(q, 0)["uncoupled_tile_pairs"] == 0
    cam_red = ies.reduced_layout(q, 0)[0]
    for t in np.unique(q.obs_pt):           # ... and nothing but those reference views couples the two tiles
        cams = set(q.obs_cam[q.obs_pt == t].tolist())
        tiles = {s for c_ in cams if cam_red[c_] >= 0 for s in ies._tiles(6 * cam_red[c_], 6)}
        assert not {0, 2} <= tiles
    far = np.nonzero(np.isin(q.point_ref_cam, (2, 3, 4)) & (np.bincount(q.obs_pt[q.obs_cam == q.point_ref_cam[q.obs_pt]], minlength=len(q.points)) == 0))[0]
    assert len(far) == 6


# ---------------------------------------------------------------- admission
@pytest.mark.parametrize("name", list(ies.CASES))
def test_case_is_admitted(name):
    case = ies.CASES[name]
    ok, dev, wander, acc = ies.admission(case)
    print("%s: %d iterations, accepted %s, wander bound %.3f; two oracle runs in units of the GPU tolerance: %s"
          % (name, case.iters, acc, wander, dev))
    assert ok, (name, dev, wander)
    assert case.iters == 1 or name in ies.TILE_CASES or case.iters == ies.ITERS.get(name, ies.ITERATIONS)


def test_the_case_table_keeps_what_it_must():
    C = ies.CASES
    for m in MODELS:                        # every model: the default case and a free-intrinsics case, with the reference-only tracks
        assert "model%d-default" % m in C and "model%d-intr11" % m in C and "model%d-cauchy+intr3f" % m in C
        assert idp.reference_only(C["model%d-default" % m].problem()).sum() == 10
    assert {c.options.get("loss_function_type", 0) for c in C.values()} == set(es.LOSSES)
    # a model with a validity region runs all its iterations with the reference-only tracks in the scene
    assert C["model6-default"].iters == ies.ITERATIONS and es.branch_counts(ies.as_points_problem(C["model6-default"].problem()))["eucm_alpha_gt_half"] > 0
    for name, case in C.items():            # a shortened case has a twin that is not shortened for the same reason
        if name in ies.ITERS and not name.endswith("-observable") and not name.startswith("model7") and "intr" not in name:
            assert C[name + "-observable"].iters == ies.ITERATIONS
    assert all(n in C for n in ies.ITERS) and all(n in C for n in ies.PERTURB)


def test_oracle_starts_at_the_same_cost_in_both_forms():
    """The conversion changes the parametrisation, not the problem: the oracle's initial cost of the inverse-depth scene
    (no edits) is its cost of the scene it came from."""
    for model in MODELS:
        p = es.edge_scene(model, 1, negative_w=False)
        p.points /= p.points[:, 3:4]         # (w = 1: the orthographic model does not divide a homogeneous point by its w)
        q = idp.from_problem(p, "first")
        o = ol.default_options(); o.max_num_iterations = 0
        s, _ = ol.solve_inverse_depth(q, o)
        _, cost, _, _, _ = ol.evaluate(p, ol.default_options())
        assert abs(s.initial_cost - cost) <= 1e-9 * cost, (model, s.initial_cost, cost)
