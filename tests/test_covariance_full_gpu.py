"""GPU: theia_hip_ba_covariance_full -- the camera and point blocks of (J'J)^-1 of problems in which cameras and points
are both free -- against numpy's dense inverse of J'J assembled from the oracle's Jets (tests/covariance_ref.py).

Tolerance of every comparison: max|got - ref| <= 1e4 * cond(J'J) * 2^-52 * max|ref block|, cond from the reference matrix
(tests/test_covariance_full.py asserts cond <= 1e6, <= 1e9 with free intrinsics, for every scene here).  Each test prints
its worst error as a fraction of that bound."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba, sfm, synth
from tests import covariance_ref as cr
from tests import invdepth as idp
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_cache = {}


def solved_scene(name, **extra):
    """(solved problem, device options, reference camera blocks, reference point blocks, cond, V_p^-1 blocks): one solve
    and one dense inverse per scene, shared by the tests."""
    key = (name, tuple(sorted(extra.items())))
    if key not in _cache:
        build, fields, free_intr = cr.GPU_SCENES[name]
        o, oo = cr.options(**fields, **extra)
        p = build()
        with ba.BaHandle(p, o) as h:
            s, _ = h.run()
            h.download()
        assert s.success
        J, lay = cr.dense_jacobian(p, oo, free_intr)
        H = J.T @ J
        rank_deficient = np.linalg.matrix_rank(H) < lay.ncol
        cams, pts, cond = ({}, {}, np.inf) if rank_deficient else cr.blocks_from_dense_inverse(J, lay)
        vinv = {} if rank_deficient else cr.blocks_from_schur_form(J, lay)[2]
        _cache[key] = (p, o, cams, pts, cond, vinv)
    return _cache[key]


def worst_ratio(got, ref, cond):
    """max over the blocks of |got - ref| / (1e4 * cond * eps * max|ref block|): <= 1 passes."""
    return max(np.abs(got[k] - ref[k]).max() / (1e4 * cond * EPS * np.abs(ref[k]).max()) for k in ref)


def same_blocks(a, b, cond):
    """Two calls see reduced systems that differ by the summation order of the assembly's FP64 atomics: an ulp-sized
    relative perturbation of S, amplified by at most cond."""
    return np.abs(a - b).max() <= 100.0 * cond * EPS * np.abs(b).max()


def check_against_reference(label, cc, pc, cams, pts, cond):
    rc, rp = worst_ratio(cc, cams, cond), worst_ratio(pc, pts, cond)
    print(f"{label}: cond(J'J) {cond:.3g}, bound {1e4 * cond * EPS:.2e} relative, worst cameras {rc:.3g}, worst points {rp:.3g} of the bound")
    assert rc <= 1.0 and rp <= 1.0
    for c in range(cc.shape[0]):
        if c not in cams:
            assert np.all(cc[c] == 0.0)
    for q in range(pc.shape[0]):
        if q not in pts:
            assert np.all(pc[q] == 0.0)


def test_all_blocks_match_the_dense_inverse():
    p, o, cams, pts, cond, vinv = solved_scene("basic")
    with ba.BaHandle(p.copy(), o) as h:
        cc, pc = h.covariance_full(cameras=True, points=True)
    assert len(cams) == 4 and len(pts) == 40
    check_against_reference("basic", cc, pc, cams, pts, cond)
    for c in cams:
        assert np.array_equal(cc[c], cc[c].T) and np.all(np.linalg.eigvalsh(cc[c]) > 0)
    for q in pts:
        assert np.array_equal(pc[q], pc[q].T) and np.all(np.linalg.eigvalsh(pc[q]) > 0)
        # the coupling with the cameras is in: V_p^-1 alone is a different matrix
        assert np.abs(pc[q] - vinv[q]).max() > 1e-3 * np.abs(pc[q]).max()


def test_chunked_solves_and_selections():
    """n = 72 crosses a 64-tile edge; 16 unit vectors per solve (five chunks); selected blocks equal the unselected call's."""
    p, o, cams, pts, cond, _ = solved_scene("tile_edge")
    with ba.BaHandle(p.copy(), o) as h:
        assert h.plan_info()["n"] == 72
        cc, pc = h.covariance_full(cameras=True, points=True, max_rhs_columns=16)
        check_against_reference("tile_edge", cc, pc, cams, pts, cond)
        cs, ps = h.covariance_full(cameras=True, points=True, view_sel=[1, 5], track_sel=[0, 7, 33], max_rhs_columns=16)
        c1, p1 = h.covariance_full(cameras=True, points=True)     # the library's chunk
    for v in range(14):
        if v in (1, 5):
            assert same_blocks(cs[v], cc[v], cond) and np.abs(cc[v]).max() > 0
        else:
            assert np.all(cs[v] == 0.0)
    for t in range(80):
        if t in (0, 7, 33):
            assert same_blocks(ps[t], pc[t], cond) and np.abs(pc[t]).max() > 0
        else:
            assert np.all(ps[t] == 0.0)
    assert all(same_blocks(c1[v], cc[v], cond) for v in cams) and all(same_blocks(p1[t], pc[t], cond) for t in pts)


def test_huber_loss_mixed_models_and_sqrt_information():
    p, o, cams, pts, cond, _ = solved_scene("robust")
    assert o.loss_function_type == 1 and len(set(p.group_model.tolist())) == 2 and p.obs_sqrt_info is not None
    with ba.BaHandle(p.copy(), o) as h:
        cc, pc = h.covariance_full(cameras=True, points=True)
    check_against_reference("robust", cc, pc, cams, pts, cond)


def test_free_intrinsics():
    """FOCAL_LENGTH | RADIAL_DISTORTION on two shared groups: the intrinsics columns are in J (and in S), their frozen
    slots are empty rows of the reduced system; the reference's J takes J_intr from evaluate_ex."""
    p, o, cams, pts, cond, vinv = solved_scene("intrinsics")
    with ba.BaHandle(p.copy(), o) as h:
        assert h.plan_info()["n"] == 20 + 6 * 7
        cc, pc = h.covariance_full(cameras=True, points=True)
        cs, ps = h.covariance_full(cameras=True, points=True, view_sel=[2], track_sel=[11, 64])
    check_against_reference("intrinsics", cc, pc, cams, pts, cond)
    assert same_blocks(cs[2], cc[2], cond)
    for t in (11, 64):
        assert same_blocks(ps[t], pc[t], cond)
    assert np.count_nonzero(np.abs(ps).reshape(120, -1).max(axis=1)) == 2


def test_long_tracks():
    """Three tracks of 70 observations (the long-track path, the pair-tile loop) among 60 tracks of 8 .. 36."""
    p, o, cams, pts, cond, _ = solved_scene("long_tracks")
    with ba.BaHandle(p.copy(), o) as h:
        assert h.plan_info()["slow_path_tracks"] >= 3
        cc, pc = h.covariance_full(cameras=True, points=True)
        c2, p2 = h.covariance_full(cameras=True, points=True)
    check_against_reference("long_tracks", cc, pc, cams, pts, cond)
    assert all(np.abs(pc[q]).max() > 0 for q in (60, 61, 62))
    assert all(same_blocks(p2[q], pc[q], cond) for q in pts) and all(same_blocks(c2[c], cc[c], cond) for c in cams)


def test_partially_constant_camera_and_constant_point():
    p, o, cams, pts, cond, _ = solved_scene("partial_constant")
    with ba.BaHandle(p.copy(), o) as h:
        cc, pc = h.covariance_full(cameras=True, points=True)
    check_against_reference("partial_constant", cc, pc, cams, pts, cond)
    assert np.all(cc[0] == 0.0) and np.all(pc[5] == 0.0)
    assert np.all(cc[1][:3, :] == 0.0) and np.all(cc[1][:, :3] == 0.0) and np.all(np.linalg.eigvalsh(cc[1][3:, 3:]) > 0)


def test_unparametrised_homogeneous_points():
    """pd = 4: the projection does not depend on the scale of X, J'J has one null direction per point -- the reference
    matrix decides, and the entry then reports the rank deficiency as ceres::Covariance::Compute would."""
    p, o, cams, pts, cond, _ = solved_scene("basic", use_homogeneous_point_parametrization=0)
    with ba.BaHandle(p.copy(), o) as h:
        assert h.pd == 4
        if not pts:      # rank deficient by the reference
            with pytest.raises(capi.TheiaHipError) as e:
                h.covariance_full(cameras=True, points=True)
            assert e.value.code == capi.THEIA_HIP_ERR_INTERNAL and "rank deficient" in str(e.value)
        else:
            cc, pc = h.covariance_full(cameras=True, points=True)
            check_against_reference("pd4", cc, pc, cams, pts, cond)


def test_errors_leave_the_handle_usable():
    p = cr.scene_basic()
    o = ba.default_options()
    with ba.BaHandle(p.copy(), o) as h:
        fresh_cost = h.run()[0].final_cost
    # a track with one observation: V_p has rank 2
    one = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, np.vstack([p.points, [[0.2, 0.1, -0.3, 1.0]]]),
                           np.vstack([p.obs_uv, [[900.0, 500.0]]]), np.append(p.obs_cam, 1).astype(np.int32),
                           np.append(p.obs_pt, 40).astype(np.int32), cam_const=p.cam_const)
    with ba.BaHandle(one.copy(), o) as h:
        with pytest.raises(capi.TheiaHipError) as e:
            h.covariance_full(cameras=True, points=True)
        assert e.value.code == capi.THEIA_HIP_ERR_INTERNAL and "rank deficient (ceres::Covariance::Compute fails)" in str(e.value)
        cc, pc = h.covariance_full(cameras=True, points=True, track_sel=list(range(40)))   # the other tracks are fine
        assert np.abs(pc[:40]).reshape(40, -1).max(axis=1).min() > 0 and np.all(pc[40] == 0.0)
        with ba.BaHandle(one.copy(), o) as h2:
            ref_cost = h2.run()[0].final_cost
        assert abs(h.run()[0].final_cost - ref_cost) <= 1e-9 * ref_cost          # after a failed and a successful call
    with ba.BaHandle(p.copy(), o) as h:
        h.covariance_full(cameras=True, points=True)
        h.covariance_full(cameras=True, view_sel=[1])
        assert abs(h.run()[0].final_cost - fresh_cost) <= 1e-9 * fresh_cost
        with pytest.raises(capi.TheiaHipError) as e:
            h.covariance_full(cameras=True, view_sel=[6])
        assert e.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    with ba.BaHandle(p.copy(), o) as h:
        h.set_shard(0, 2)
        with pytest.raises(capi.TheiaHipError) as e:
            h.covariance_full(cameras=True, points=True)
        assert e.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED
    with ba.BaHandle(idp.make(4, 40, seed=2), ba.default_options()) as h:
        with pytest.raises(capi.TheiaHipError) as e:
            h.covariance_full(cameras=True, points=True)
        assert e.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED


def test_mirror_partial_reconstruction_with_cov():
    """BundleAdjustPartialReconstructionWithCov, four of ten views free: the variance factor is
    2 * final_cost / (2 * #observations - #free parameters), the dictionaries are the handle's blocks times the factor."""
    p = synth.synth_ba_v1(10, 120, seed=0xC0700009, num_groups=2)
    opts = sfm.BundleAdjustmentOptions(); opts.max_num_iterations = 30
    views, tracks = [2, 3, 4, 5], list(range(120))
    rec = sfm.Reconstruction.from_flat(p)
    summ, cv, ct, factor = sfm.BundleAdjustPartialReconstructionWithCov(opts, views, tracks, rec, cov_view_ids=[3, 5], cov_track_ids=[0, 17, 119])
    assert summ.success and sorted(cv) == [3, 5] and sorted(ct) == [0, 17, 119]
    flat = sfm._flatten(rec, views, tracks, options=opts)          # the solved state
    nobs = flat.obs_uv.shape[0]
    assert nobs == p.obs_uv.shape[0]
    expect = 2.0 * summ.final_cost / (2 * nobs - (6 * 4 + 3 * 120))
    assert abs(factor - expect) <= 1e-12 * expect
    with ba.BaHandle(flat, sfm._no_inner(opts).to_c()) as h:
        cc, pc = h.covariance_full(cameras=True, points=True)
    for v in cv:
        assert cv[v].shape == (6, 6) and np.abs(cv[v] - factor * cc[v]).max() <= 1e-9 * np.abs(cv[v]).max() and np.abs(cc[v]).max() > 0
    for t in ct:
        assert ct[t].shape == (3, 3) and np.abs(ct[t] - factor * pc[t]).max() <= 1e-9 * np.abs(ct[t]).max() and np.abs(pc[t]).max() > 0
    assert np.all(cc[[0, 1, 6, 7, 8, 9]] == 0.0)                  # cameras reached only through AddTrack are constant
    # and against the reference
    J, lay = cr.dense_jacobian(flat, ol.default_options())
    cams, pts, cond = cr.blocks_from_dense_inverse(J, lay)
    check_against_reference("mirror", cc, pc, cams, pts, cond)
    # the full-reconstruction variant goes through the same path; with every view free the gauge is free and J'J singular:
    # either the pivots catch it (success False, empty dictionaries) or the blocks are noise -- it must not raise
    s2, cv2, ct2, f2 = sfm.BundleAdjustReconstructionWithCov(opts, sfm.Reconstruction.from_flat(p), cov_view_ids=[0], cov_track_ids=[1])
    assert (s2.success and sorted(cv2) == [0] and sorted(ct2) == [1]) or (not s2.success and cv2 == {} and ct2 == {})
