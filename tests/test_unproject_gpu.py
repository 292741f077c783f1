"""GPU: theia_hip_unproject and the camera module against the restatement of tests/unproject_ref.py, against the existing
pinhole code, and against itself (one wave of eight models; every output alone); then end to end on a fisheye scene."""
import functools
import os

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import ba, camera, ransac, sfm, twoview
from pytheiasfm_amd import incremental as inc
from tests import ba_edge_scenes as es
from tests import unproject_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "camera_models.npz"))
BLOCK = 256                                  # k_unproject's workgroup
SIZES = (1, 63, 64, 65, BLOCK + 1)           # the wave edge, one past a workgroup
ALL = ("camera_point", "normalized", "world_ray", "world_ray_unit", "status", "iterations")
BITWISE = (0, 1, 4, 5, 6, 7)                 # + - * / and sqrt only


def intrinsics(model):
    """The golden file's intrinsics; for the orthographic model a distortion that stays in range at its magnification."""
    k = np.zeros(10)
    v = [1.5, 1.0, 0.0, 320.0, 240.0, 1e-6, 1e-9] if model == 7 else GOLDEN[f"m{model}_intr"]
    k[:len(v)] = v
    return k


def principal_point(model, k):
    return (k[2], k[3]) if model in (3, 4) else (k[3], k[4])


def grid(model, n):
    """n pixels: the principal point, then a grid over the image (twice the principal point on each side), borders included."""
    cx, cy = principal_point(model, intrinsics(model))
    cols = int(np.ceil(np.sqrt(max(n - 1, 1)))) + 1
    k = np.arange(n - 1)
    rest = np.column_stack([(k % cols) / (cols - 1) * 2.0 * cx, (k // cols) / (cols - 1) * 2.0 * cy])
    return np.ascontiguousarray(np.vstack([[cx, cy], rest]))


@functools.lru_cache(maxsize=None)
def restated(model, n):
    out = ref.unproject(model, intrinsics(model), grid(model, n))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device(model, n):
    out = camera.unproject(grid(model, n), None, [0], None, intrinsics(model), [model],
                           ("camera_point", "normalized", "status", "iterations"), summary=True)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_values(a, b):
    """Equal doubles with NaN in the same places (a NaN's payload is not part of any contract)."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b)) \
        and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------ 5. single-model calls
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("model", range(8))
def test_single_model_against_the_restatement(model, n):
    want, got = restated(model, n), device(model, n)
    assert got["camera_point"].shape == (n, 3) and got["normalized"].shape == (n, 2)
    assert np.array_equal(got["camera_point"][0], [0.0, 0.0, 1.0])              # the principal point
    s = got["summary"]
    assert s["num_invalid"] == np.count_nonzero(~(got["status"] & 1).astype(bool))
    assert s["num_not_converged"] == np.count_nonzero(~(got["status"] & 2).astype(bool))
    assert s["max_iterations"] == got["iterations"].max()
    if model in BITWISE:
        for name in ("camera_point", "normalized"):
            assert same_values(got[name], want[name]), (name, np.nanmax(np.abs(got[name] - want[name])))
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"])
    elif model == 2:
        # the two sides differ by the rounding of atan2: they may leave the loop one trip apart, and a trip near the exit moves the
        # iterate by less than the reference's own 1e-10
        worst = max(np.abs(got[name] - want[name]).max() for name in ("camera_point", "normalized"))
        trips = np.abs(got["iterations"].astype(int) - want["iterations"].astype(int)).max()
        print(f"fisheye n={n}: max |diff| {worst:.3e}, max trip difference {trips}")
        assert worst <= 2e-10 and trips <= 1
        assert np.array_equal(got["status"] & 1, want["status"] & 1)
    else:
        # tan is a few ulp on both sides and its condition number is below 4 for r_d omega <= 1.2: about 1e-14
        k = intrinsics(3)
        px = grid(3, n)
        rd = np.hypot((px[:, 0] - k[2]) / k[0], (px[:, 1] - k[3]) / (k[0] * k[1]))
        assert (rd * k[4]).max() <= 1.2
        worst = max((np.abs(got[name] - want[name]) / np.maximum(np.abs(want[name]), 1e-300)).max() for name in ("camera_point", "normalized"))
        print(f"FOV n={n}: max relative difference {worst:.3e}")
        assert worst <= 1e-12
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"])


def test_the_grids_take_every_path():
    """What the shapes above are chosen for: the loops run different trip counts inside one wave, the orthographic loop runs
    its 100 trips, the FOV grid has pixels in both branches of omega >= 1e-3."""
    for model in (0, 1, 2):
        it = restated(model, BLOCK + 1)["iterations"]
        assert it.min() == 1 and it.max() > 3 and len(set(it[:64].tolist())) >= 3, model
    o = restated(7, BLOCK + 1)
    assert o["iterations"].max() == 100 and np.count_nonzero(o["status"] == 1) > 0 and np.count_nonzero(o["status"] == 3) > 0
    k = intrinsics(3)
    assert {ref.fov_branch(k, u, v) for u, v in grid(3, BLOCK + 1)} == {1, 2}


def test_fov_small_omega_branch_on_the_device():
    k = intrinsics(3); k[4] = 5e-4
    px = grid(3, 65)
    got = camera.unproject(px, None, [0], None, k, [3], ("camera_point",))["camera_point"]
    assert same_values(got, ref.unproject(3, k, px)["camera_point"])          # no tan in this branch: the same bits


# ------------------------------------------------------------------ 6. model 0 against the existing host code
def test_pinhole_equals_ransac_camera_pixel_to_normalized():
    k = intrinsics(0)
    cam = ransac.Camera([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], k, 0)
    px = grid(0, BLOCK + 1)
    host = np.array([cam.pixel_to_normalized(p) for p in px])
    assert same_values(device(0, BLOCK + 1)["normalized"], host)
    assert same_values(camera.PixelToNormalizedCoordinates(cam, px)[:, :2], host)


# ------------------------------------------------------------------ 7. one wave, eight models
def _mixed_inputs(n, planted):
    """Observation k belongs to camera k % 8 = group k % 8 = model k % 8; its pixel is the one the single-model grid of its
    model has at its place in that model's sub-list."""
    px = np.empty((n, 2))
    for m in range(8):
        rows = np.arange(m, n, 8)
        px[rows] = grid(m, BLOCK + 1)[3: 3 + len(rows)]
    if planted:
        k5, k0 = intrinsics(5), intrinsics(0)
        # double sphere, alpha = 0.55: invalid from r2 >= 10 on -- 2000 px from the centre at f = 600
        px[29] = [k5[3] + 2000.0, k5[4]]
        # pinhole, k1 = -0.05, k2 = 0.01: at the distorted radius 30 the iterates jump between ~30 and ~0.004
        px[32] = [k0[3] + 30.0 * k0[0], k0[4]]
    return np.ascontiguousarray(px)


def _mixed_call(px, outputs=("camera_point", "normalized", "status", "iterations")):
    n = len(px)
    return camera.unproject(px, np.arange(n) % 8, np.arange(8), None, np.stack([intrinsics(m) for m in range(8)]), np.arange(8),
                            outputs, summary=True)


@pytest.mark.parametrize("n", [64, 65])
def test_one_wave_eight_models(n):
    plain, planted = _mixed_inputs(n, False), _mixed_inputs(n, True)
    a, b = _mixed_call(plain), _mixed_call(planted)
    for px, mixed in ((plain, a), (planted, b)):
        for m in range(8):
            rows = np.arange(m, n, 8)
            single = camera.unproject(px[rows], None, [0], None, intrinsics(m), [m], ("camera_point", "normalized", "status", "iterations"))
            for name in ("camera_point", "normalized", "status", "iterations"):
                assert same_bits(np.ascontiguousarray(mixed[name][rows]), single[name]), (m, name)
    # the planted lanes are what they were planted as, by the restatement too
    assert ref.pixel_to_camera(5, intrinsics(5), *planted[29])[1:] == (False, True, 0)
    assert ref.pixel_to_camera(0, intrinsics(0), *planted[32])[1:] == (True, False, 100)
    assert b["status"][29] == 2 and np.isnan(b["camera_point"][29]).all() and np.isnan(b["normalized"][29]).all()
    assert b["status"][32] == 1 and b["iterations"][32] == 100
    assert same_values(b["camera_point"][32], np.array(ref.pixel_to_camera(0, intrinsics(0), *planted[32])[0]))
    assert a["summary"]["num_invalid"] == 0 and b["summary"]["num_invalid"] == 1
    assert b["summary"]["num_not_converged"] == a["summary"]["num_not_converged"] + 1
    # ... and their neighbours did not notice
    others = np.setdiff1d(np.arange(n), [29, 32])
    for name in ("camera_point", "normalized", "status", "iterations"):
        assert same_bits(np.ascontiguousarray(a[name][others]), np.ascontiguousarray(b[name][others])), name


# ------------------------------------------------------------------ 8. world rays
def test_world_rays_over_six_cameras():
    rng = np.random.default_rng(0x3A75)
    ext = np.zeros((6, 6))
    ext[:, :3] = rng.standard_normal((6, 3))
    ext[:, 3:] = rng.standard_normal((6, 3))
    ext[::2, 3:] *= 1e-9 / np.linalg.norm(ext[::2, 3:], axis=1, keepdims=True)      # the first-order branch
    assert ((ext[::2, 3:] ** 2).sum(1) <= np.finfo(np.float64).eps).all() and ((ext[1::2, 3:] ** 2).sum(1) > 0.1).all()
    group = np.array([0, 1, 1, 0, 0, 1])                                            # pinhole (z = 1), double sphere (z != 1)
    models, ks = [0, 5], np.stack([intrinsics(0), intrinsics(5)])
    n = 131
    cam = np.arange(n) % 6
    px = np.where((group[cam] == 0)[:, None], grid(0, n), grid(5, n))
    got = camera.unproject(px, cam, group, ext, ks, models, ALL)
    worst = 0.0
    for i in range(n):
        m, k = models[group[cam[i]]], ks[group[cam[i]]]
        p = np.array(ref.pixel_to_camera(m, k, *px[i])[0])
        assert same_values(got["camera_point"][i], p)
        ray = np.array(ref.pixel_to_unit_depth_ray(m, k, ext[cam[i], 3:], *px[i]))
        bound = 1e-13 * max(1.0, np.linalg.norm(p))
        d = max(np.abs(got["world_ray"][i] - ray).max(), np.abs(got["world_ray_unit"][i] - ray / np.linalg.norm(ray)).max())
        worst = max(worst, d / bound)
        assert d <= bound, (i, d, bound)
    print(f"world rays: worst |diff| / bound {worst:.3e}")
    # without extrinsics, while no ray is asked for
    alone = camera.unproject(px, cam, group, None, ks, models, ("camera_point",))
    assert same_bits(alone["camera_point"], got["camera_point"])
    # the per-camera wrappers
    c = ransac.Camera(ext[1, :3], ext[1, 3:], ks[1], 5)
    assert same_bits(camera.PixelToUnitDepthRay(c, px[1::6]), np.ascontiguousarray(got["world_ray"][1::6]))
    assert same_bits(camera.PixelToNormalizedCoordinates(c, px[1::6]), np.ascontiguousarray(got["camera_point"][1::6]))


# ------------------------------------------------------------------ 9. optional outputs
def test_every_output_alone_and_the_empty_call():
    rng = np.random.default_rng(7)
    ext = rng.standard_normal((8, 6))
    px = _mixed_inputs(65, True)
    args = (px, np.arange(65) % 8, np.arange(8), ext, np.stack([intrinsics(m) for m in range(8)]), np.arange(8))
    full = camera.unproject(*args, outputs=ALL)
    for name in ALL:
        alone = camera.unproject(*args, outputs=(name,))
        assert list(alone) == [name] and same_bits(alone[name], full[name]), name
    none = camera.unproject(*args, outputs=(), summary=True)
    assert list(none) == ["summary"] and none["summary"]["num_invalid"] == 1 and none["summary"]["max_iterations"] == 100
    empty = camera.unproject(np.zeros((0, 2)), np.zeros(0, np.int32), args[2], ext, args[4], args[5], outputs=ALL, summary=True)
    assert [empty[name].shape for name in ALL] == [(0, 3), (0, 2), (0, 3), (0, 3), (0,), (0,)]
    assert empty["summary"]["num_invalid"] == 0 and empty["summary"]["max_iterations"] == 0


# ------------------------------------------------------------------ 10. end to end on the fisheye edge scene
@functools.lru_cache(maxsize=None)
def _fisheye_scene():
    """The fisheye edge scene at its own state, observed without noise by the oracle's projection; the observations of points
    behind their camera are left out (a pixel un-projects to z = 1)."""
    p = es.edge_scene(2)
    ok, uv = es.project_with_oracle(p, p.cam_ext, p.points)
    assert ok == 1
    front = es.camera_frame(p.cam_ext, p.points, p.obs_cam, p.obs_pt)[:, 2] > 0.0
    assert 0 < np.count_nonzero(~front) < 10
    q = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, p.points, uv[front], p.obs_cam[front], p.obs_pt[front])
    assert np.bincount(q.obs_pt, minlength=len(q.points)).min() >= 2
    return q


def test_fisheye_rays_estimate_every_track():
    q = _fisheye_scene()
    truth = q.points[:, :3] / q.points[:, 3:]
    pg = q.copy()
    pg.points[:] = [0.0, 0.0, 0.0, 1.0]
    rays = camera.ObservationRays(pg)
    assert rays.shape == (len(q.obs_uv), 3) and np.abs(np.linalg.norm(rays, axis=1) - 1.0).max() < 1e-15
    # a ray points from its camera at its point
    to_point = truth[q.obs_pt] - q.cam_ext[q.obs_cam, :3]
    to_point /= np.linalg.norm(to_point, axis=1, keepdims=True)
    assert np.linalg.norm(np.cross(rays, to_point), axis=1).max() < 1e-8 and (np.einsum("ij,ij->i", rays, to_point) > 0).all()
    bo = sfm.BundleAdjustmentOptions(); bo.max_num_iterations = 10; bo.use_inner_iterations = False
    est, counts = ba.estimate_tracks(pg, rays, bo.to_c(), 3.0, 5.0, True)
    assert est.all(), (np.flatnonzero(~est), counts)
    assert counts == {"bad_angles": 0, "failed_triangulations": 0, "bad_reprojections": 0, "ba_failures": 0}
    got = pg.points[:, :3] / pg.points[:, 3:]
    assert np.abs(got - truth).max() < 1e-6
    # the same rays from the reconstruction's arrays
    assert same_bits(camera.ObservationRays(sfm.Reconstruction.from_flat(q)), rays)


def test_fisheye_normalized_features_localise_a_view():
    q = _fisheye_scene()
    V = 6
    r = sfm.Reconstruction.from_flat(q)
    r.view_image_size = np.tile(np.array([1920, 1080], np.int32), (r.NumViews(), 1))
    r.view_focal_prior_set = np.zeros(r.NumViews(), bool)
    r.view_focal_prior_set[V] = True
    r.view_estimated[V] = False
    truth = r.cam_ext[V].copy()
    r.cam_ext[V, :3] += np.array([0.7, -0.4, 0.3])
    r.cam_ext[V, 3:6] += 0.2
    start = r.cam_ext[V].copy()
    o = inc.LocalizeViewToReconstructionOptions()          # the options of the pinhole test of this function
    o.ransac_params.min_iterations = 32
    o.ransac_params.max_iterations = 128
    o.ransac_params.seed = 11
    o.ba_options.max_num_iterations = 10
    assert np.count_nonzero(r.obs_view == V) >= 2 * o.min_num_inliers
    with pytest.raises(capi.TheiaHipError) as e:           # the mirror keeps refusing the model without the argument
        inc.LocalizeViewToReconstruction(V, o, r)
    assert e.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED
    nf = camera.NormalizedFeatures(r)
    assert nf.shape == r.obs_uv.shape
    ok, summary = inc.LocalizeViewToReconstruction(V, o, r, normalized_features=nf)
    # what the pinhole test asserts
    assert ok is True and r.view_estimated[V] and len(summary.inliers) >= o.min_num_inliers
    assert not np.array_equal(r.cam_ext[V], start)
    # and, the scene being free of noise, the pose itself: the 4 px inlier threshold spans 4 / 600 * 7 = 0.047 at the scene's
    # depth and focal length; an exact-data pose is asserted at a fiftieth of that (a rotation by 1e-3 moves a point at that
    # depth by 0.007)
    assert np.abs(r.cam_ext[V, :3] - truth[:3]).max() < 1e-3
    Rt, Rg = es.angle_axis_to_matrix(truth[3:]), es.angle_axis_to_matrix(r.cam_ext[V, 3:6])
    assert np.abs(Rt - Rg).max() < 1e-3


# ------------------------------------------------------------------ 11. NormalizeFeatures
def _pinhole_prior(focal, size=(0, 0), pp=None, aspect=None, skew=None, zero_radial=False):
    p = twoview.CameraIntrinsicsPrior()
    p.image_width, p.image_height = size
    if focal is not None:
        p.focal_length.is_set = True; p.focal_length.value = [focal]
    if pp is not None:
        p.principal_point.is_set = True; p.principal_point.value = list(pp)
    if aspect is not None:
        p.aspect_ratio.is_set = True; p.aspect_ratio.value = [aspect]
    if skew is not None:
        p.skew.is_set = True; p.skew.value = [skew]
    if zero_radial:
        p.radial_distortion.is_set = True
    return p


@pytest.mark.parametrize("reset", [False, True])
def test_normalize_features_equals_the_pinhole_mirror(reset):
    rng = np.random.default_rng(0x2F)
    corr = rng.uniform(0.0, 1200.0, size=(BLOCK + 1, 4))
    p1 = _pinhole_prior(None if reset else 810.5, size=(1280, 960), aspect=1.01, skew=0.3)
    p2 = _pinhole_prior(1234.25, pp=(601.5, 333.25), zero_radial=True)
    want = twoview.NormalizeFeatures(p1, p2, corr)
    got = camera.NormalizeFeatures(p1, p2, corr)
    assert same_bits(got, want)
    if reset:      # both focal lengths are 1: only the principal point (and the first view's skew and aspect ratio) is removed
        assert np.array_equal(got[:, 2:], corr[:, 2:] - [601.5, 333.25])


def test_normalize_features_of_two_other_models():
    rng = np.random.default_rng(0x30)
    corr = rng.uniform(200.0, 1000.0, size=(65, 4))
    p1 = _pinhole_prior(500.0, pp=(640.0, 480.0), aspect=1.01); p1.camera_intrinsics_model_type = "FISHEYE"
    p1.radial_distortion.is_set = True; p1.radial_distortion.value = [-0.01, 0.002, -0.0003, 4e-05]
    p2 = _pinhole_prior(600.0, pp=(640.0, 360.0)); p2.camera_intrinsics_model_type = "DOUBLE_SPHERE"
    p2.radial_distortion.is_set = True; p2.radial_distortion.value = [0.55, -0.2, 0.0, 0.0]        # alpha, xi
    got = camera.NormalizeFeatures(p1, p2, corr)
    assert np.array_equal(camera.IntrinsicsFromPrior(p1)[1], intrinsics(2)) and np.array_equal(camera.IntrinsicsFromPrior(p2)[1], intrinsics(5))
    left = ref.unproject(2, intrinsics(2), corr[:, :2])["normalized"]
    right = ref.unproject(5, intrinsics(5), corr[:, 2:])["normalized"]
    assert np.abs(got[:, :2] - left).max() <= 2e-10          # the fisheye bound of test 5
    assert same_values(np.ascontiguousarray(got[:, 2:]), right)
