"""CPU: the restatement of the eight PixelToCameraCoordinates (tests/unproject_ref.py) against the oracle's projection and
against hand-worked values; camera.IntrinsicsFromPrior; the refusals of theia_hip_unproject that return before a device is
touched, and its declaration against the ctypes signature."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import camera, twoview
from tests import unproject_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "camera_models.npz"))
INV = capi.THEIA_HIP_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ 1. round trip against the oracle's projection
@pytest.mark.parametrize("model", range(8))
def test_round_trip_against_the_oracles_projection(model):
    """The golden tuples hold the oracle's residual sqrt_info * (projection - uv) with sqrt_info = [1 + 0.1 (i % 3), 0.9]:
    the projected pixel is uv + res / sqrt_info, and its un-projection must be parallel to the camera-frame point (orthographic:
    equal in x and y).  The camera-frame point is the one the projection was taken of, Camera::ProjectPoint's
    R (X - w c) (camera.cc:207-210): parallel to R (X / w - c), and for the orthographic model, which does not divide by the
    depth, w times it -- the golden points carry w != 1.  Left out: invalid projections, loops that did not converge, and
    points behind the camera for the models that return z = 1 (0-4) or whose projection folds them (6)."""
    g = {k: GOLDEN[f"m{model}_{k}"] for k in ("ext", "X", "uv", "ok", "res", "intr")}
    used, worst = 0, 0.0
    for i in range(64):
        if not g["ok"][i]:
            continue
        pixel = g["uv"][i] + g["res"][i] / np.array([1.0 + 0.1 * (i % 3), 0.9])
        R = np.array(ref.angle_axis_to_rotation_matrix(g["ext"][i, 3:6].tolist()))
        q = R @ (g["X"][i, :3] - g["X"][i, 3] * g["ext"][i, :3])
        if model in (0, 1, 2, 3, 4, 6) and q[2] <= 0.0:
            continue
        p, valid, converged, _ = ref.pixel_to_camera(model, g["intr"], pixel[0], pixel[1])
        if not converged:
            continue
        assert valid, i
        p = np.array(p)
        if model == 7:
            err = np.linalg.norm(p[:2] - q[:2]) / np.linalg.norm(q[:2])
        else:
            err = np.linalg.norm(np.cross(p, q)) / (np.linalg.norm(p) * np.linalg.norm(q))
        worst = max(worst, err)
        used += 1
    print(f"model {model}: {used} tuples used, worst {worst:.3e}")
    assert used >= 54, used
    assert worst <= 1e-8, worst


# ------------------------------------------------------------------ 2. hand-worked values
K = {   # intrinsics with every slot in use
    0: [500.0, 1.02, 0.3, 320.0, 240.0, -0.1, 0.02],
    1: [500.0, 1.02, 0.3, 320.0, 240.0, -0.1, 0.02, 0.001, 0.002, -0.001],
    2: [300.0, 1.02, 0.3, 320.0, 240.0, 0.01, -0.002, 0.001, 0.0005],
    3: [400.0, 1.02, 320.0, 240.0, 0.9],
    4: [500.0, 1.02, 320.0, 240.0, -1e-7],
    5: [300.0, 1.02, 0.3, 320.0, 240.0, -0.25, 0.75],
    6: [300.0, 1.02, 0.3, 320.0, 240.0, 0.6, 1.1],
    7: [80.0, 1.02, 0.3, 320.0, 240.0, 1e-6, 1e-9],
}


@pytest.mark.parametrize("model", range(8))
def test_principal_point_is_the_optical_axis(model):
    k = K[model]
    cx, cy = (k[2], k[3]) if model in (3, 4) else (k[3], k[4])
    p, valid, converged, trips = ref.pixel_to_camera(model, k, cx, cy)
    assert p == (0.0, 0.0, 1.0) and valid and converged
    # the fixed points stop after one trip: pinhole-like loops by a zero difference, the fisheye by its r < 1e-8 return
    assert trips == (1 if model in ref.ITERATIVE else 0)


@pytest.mark.parametrize("model", [0, 1, 7])
def test_zero_distortion_is_the_closed_form_in_one_trip(model):
    f, a, s, cx, cy = 500.0, 1.25, 0.5, 320.0, 240.0
    u, v = 401.0, 133.0
    p, valid, converged, trips = ref.pixel_to_camera(model, [f, a, s, cx, cy], u, v)
    if model == 7:
        y = v - cy
        x = u - cx - y * s
        expected = (x / f, y / (f * a), 1.0)
    else:
        y = (v - cy) / (f * a)
        expected = ((u - cx - y * s) / f, y, 1.0)
    assert p == expected and valid and converged and trips == 1
    # the numbers, by hand: y = -107 / 625 = -0.1712, x = (81 + 0.0856) / 500 = 0.1621712
    if model != 7:
        assert p[1] == -107.0 / 625.0 and abs(p[0] - 0.1621712) < 1e-15


def test_fisheye_without_distortion_is_tan_theta():
    # theta_d = theta: the undistorted radius is tan(r_d); r_d = 0.5 along x
    p, valid, converged, trips = ref.pixel_to_camera(2, [200.0, 1.0, 0.0, 320.0, 240.0], 420.0, 240.0)
    assert valid and converged and 1 < trips < 100
    assert abs(p[0] - math.tan(0.5)) < 1e-9 and p[1] == 0.0 and p[2] == 1.0


def test_fov_three_branches():
    f, cx, cy = 400.0, 320.0, 240.0
    # omega < 1e-3: r_u = omega^2 r_d^2 / 3 - omega^2 / 12 + 1
    k = [f, 1.0, cx, cy, 5e-4]
    assert ref.fov_branch(k, 520.0, 240.0) == 0
    p = ref.pixel_to_camera(3, k, 520.0, 240.0)[0]
    omega, rd2 = 5e-4, 0.5 * 0.5
    assert p == (((omega * omega * rd2) / 3.0 - omega * omega / 12.0 + 1.0) * 0.5, 0.0, 1.0)
    assert abs(p[0] / 0.5 - 1.0) < 1e-7
    # r_d^2 < 1e-3: r_u = omega (omega^2 r_d^2 + 3) / (6 tan(omega / 2)); r_d = 0.01
    k = [f, 1.0, cx, cy, 0.9]
    assert ref.fov_branch(k, 324.0, 240.0) == 1
    p = ref.pixel_to_camera(3, k, 324.0, 240.0)[0]
    assert p == ((0.9 * (0.9 * 0.9 * (0.01 * 0.01) + 3.0)) / (6.0 * math.tan(0.45)) * 0.01, 0.0, 1.0)
    # else: tan(r_d omega) / (2 r_d tan(omega / 2)); r_d = 0.5 along y
    assert ref.fov_branch(k, 320.0, 440.0) == 2
    p, valid, converged, trips = ref.pixel_to_camera(3, k, 320.0, 440.0)
    assert p == (0.0, math.tan(0.45) / (2.0 * 0.5 * math.tan(0.45)) * 0.5, 1.0) and p[1] == 0.5
    assert valid and converged and trips == 0
    # the two series agree with the tan form next to their thresholds
    exact = math.tan(0.01 * 0.9) / (2.0 * 0.01 * math.tan(0.45))
    assert abs(ref.pixel_to_camera(3, k, 324.0, 240.0)[0][0] / 0.01 - exact) < 1e-8


def test_division_undistortion_scales_in_pixels():
    f, a, cx, cy, kd = 500.0, 1.25, 320.0, 240.0, -1e-6
    p, valid, converged, trips = ref.pixel_to_camera(4, [f, a, cx, cy, kd], 620.0, 640.0)
    und = 1.0 / (1.0 + kd * (300.0 * 300.0 + 400.0 * 400.0))      # r_d^2 = 250000 px^2: 1 / 0.75
    assert p == (300.0 * und / f, 400.0 * und / (f * a), 1.0) and valid and converged and trips == 0
    assert abs(p[0] - 0.8) < 1e-15 and abs(p[1] - 400.0 / 0.75 / 625.0) < 1e-15


def test_double_sphere_on_both_sides_of_its_bound():
    # alpha = 0.6: invalid from r2 >= 1 / (2 alpha - 1) on.  f = 1, centre 0: the pixel is the distorted point
    alpha, xi = 0.6, -0.2
    k = [1.0, 1.0, 0.0, 0.0, 0.0, xi, alpha]
    bound = 1.0 / (2.0 * alpha - 1.0)
    r = math.sqrt(bound)
    while r * r < bound:            # a radius whose square is the bound itself, or the first double above it
        r = math.nextafter(r, math.inf)
    inside = math.nextafter(r, 0.0)
    while inside * inside >= bound:
        inside = math.nextafter(inside, 0.0)
    p, valid, converged, trips = ref.pixel_to_camera(5, k, r, 0.0)
    assert not valid and converged and trips == 0 and all(math.isnan(c) for c in p)
    p, valid, _, _ = ref.pixel_to_camera(5, k, inside, 0.0)
    assert valid and not any(math.isnan(c) for c in p)
    # exactly on the bound: 2 alpha - 1 = 0.25 is exact at alpha = 0.625, bound = 4, r = 2
    k[6] = 0.625
    assert 1.0 / (2.0 * 0.625 - 1.0) == 4.0
    assert not ref.pixel_to_camera(5, k, 2.0, 0.0)[1]               # r2 == bound: `>=` is invalid
    assert ref.pixel_to_camera(5, k, math.nextafter(2.0, 0.0), 0.0)[1]
    assert ref.pixel_to_camera(5, k, 0.0, -2.0)[1] is False
    # a value by hand, alpha = 0.5, xi = 0, r = 1: sqrt2 = 1, norm2 = 1, mz = 0.75, k = sqrt(mz^2 + r2) / (mz^2 + r2) = 0.8
    p = ref.pixel_to_camera(5, [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.5], 1.0, 0.0)[0]
    assert p == (0.8, 0.0, 0.8 * 0.75)


def test_extended_unified_on_both_sides_of_its_bound_and_its_clamp():
    # alpha = 0.6, beta = 1.1: invalid from r2 >= 1 / ((alpha - gamma) beta) on
    alpha, beta = 0.6, 1.1
    k = [1.0, 1.0, 0.0, 0.0, 0.0, alpha, beta]
    bound = 1.0 / ((alpha - (1.0 - alpha)) * beta)
    r = math.sqrt(bound)
    while r * r < bound:
        r = math.nextafter(r, math.inf)
    inside = math.nextafter(r, 0.0)
    while inside * inside >= bound:
        inside = math.nextafter(inside, 0.0)
    p, valid, converged, trips = ref.pixel_to_camera(6, k, 0.0, r)
    assert not valid and converged and trips == 0 and all(math.isnan(c) for c in p)
    p, valid, _, _ = ref.pixel_to_camera(6, k, 0.0, inside)
    assert valid and abs(math.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2) - 1.0) < 1e-15
    # exactly on the bound: alpha = 0.625, beta = 1: (alpha - gamma) beta = 0.25, bound = 4
    k = [1.0, 1.0, 0.0, 0.0, 0.0, 0.625, 1.0]
    assert 1.0 / ((0.625 - (1.0 - 0.625)) * 1.0) == 4.0
    assert not ref.pixel_to_camera(6, k, 2.0, 0.0)[1]
    assert ref.pixel_to_camera(6, k, math.nextafter(2.0, 0.0), 0.0)[1]
    # the clamp: alpha = 0.5 (no domain test), beta = 4 / r2 makes tmp1 = 1 - alpha^2 beta r2 = 0, so k = 0 and the norm is r;
    # r = 2^-41 < 1e-12 is clamped: the result is (r / 1e-12, 0, 0), not a unit vector
    r = 2.0 ** -41
    k = [1.0, 1.0, 0.0, 0.0, 0.0, 0.5, 4.0 / (r * r)]
    p, valid, converged, _ = ref.pixel_to_camera(6, k, r, 0.0)
    assert valid and converged and p == (r / 1e-12, 0.0, 0.0) and p[0] < 1.0


def test_pinhole_that_does_not_settle_returns_the_100th_iterate():
    # k1 = -0.5 at the distorted radius 0.6: x <- 0.6 / (1 - 0.5 x^2) has no fixed point (x - 0.5 x^3 peaks at 0.544 < 0.6)
    k = [1.0, 1.0, 0.0, 0.0, 0.0, -0.5, 0.0]
    p, valid, converged, trips = ref.pixel_to_camera(0, k, 0.6, 0.0)
    assert valid and not converged and trips == 100
    x = 0.6
    for _ in range(100):
        x = 0.6 / (1.0 + x * x * (-0.5 + 0.0 * (x * x)))
    assert p[0] == x and p[1] == 0.0 and p[2] == 1.0
    # and one that settles: radius 0.3
    p, valid, converged, trips = ref.pixel_to_camera(0, k, 0.3, 0.0)
    assert converged and 1 < trips < 100 and abs(p[0] * (1.0 - 0.5 * p[0] ** 2) - 0.3) < 1e-10


def test_world_ray_is_the_transposed_rotation():
    # a quarter turn about z: R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]], R' (x, y, 1) = (y, -x, 1)
    w = [0.0, 0.0, math.pi / 2.0]
    ray = ref.pixel_to_unit_depth_ray(0, [1.0, 1.0, 0.0, 0.0, 0.0], w, 0.25, -0.5)
    assert abs(ray[0] + 0.5) < 1e-15 and abs(ray[1] + 0.25) < 1e-15 and ray[2] == 1.0
    # the first-order branch: R = I + [w]x
    ray = ref.pixel_to_unit_depth_ray(0, [1.0, 1.0, 0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], 0.25, -0.5)
    assert ray == (0.25, -0.5 + 1e-9, 1.0 + 0.5e-9)


# ------------------------------------------------------------------ 3. IntrinsicsFromPrior
def _prior(name):
    p = twoview.CameraIntrinsicsPrior()
    p.camera_intrinsics_model_type = name
    p.tangential_distortion = twoview.Prior(2)
    return p


def _everything(name):
    p = _prior(name)
    p.image_width, p.image_height = 640, 480
    p.focal_length.is_set = True; p.focal_length.value = [450.0]
    p.principal_point.is_set = True; p.principal_point.value = [321.0, 239.0]
    p.aspect_ratio.is_set = True; p.aspect_ratio.value = [1.01]
    p.skew.is_set = True; p.skew.value = [0.2]
    p.radial_distortion.is_set = True; p.radial_distortion.value = [0.11, 0.22, 0.33, 0.44]
    p.tangential_distortion.is_set = True; p.tangential_distortion.value = [0.55, 0.66]
    return p


def _k(*values):
    k = np.zeros(10)
    k[:len(values)] = values
    return k


# (model id, nothing set, only the image size 640 x 480 set, everything set)
PRIOR_CASES = {
    "PINHOLE": (0, _k(1, 1), _k(768, 1, 0, 320, 240), _k(450, 1.01, 0.2, 321, 239, 0.11, 0.22)),
    "PINHOLE_RADIAL_TANGENTIAL": (1, _k(1, 1), _k(768, 1, 0, 320, 240), _k(450, 1.01, 0.2, 321, 239, 0.11, 0.22, 0.33, 0.55, 0.66)),
    "FISHEYE": (2, _k(1, 1), _k(256, 1, 0, 320, 240), _k(450, 1.01, 0.2, 321, 239, 0.11, 0.22, 0.33, 0.44)),     # 0.4 max(w, h)
    "FOV": (3, _k(1, 1, 0, 0, 0.75), _k(768, 1, 320, 240, 0.75), _k(450, 1.01, 321, 239, 0.11)),                # no skew slot
    "DIVISION_UNDISTORTION": (4, _k(1, 1), _k(768, 1, 320, 240, 0), _k(450, 1.01, 321, 239, 0.11)),
    "DOUBLE_SPHERE": (5, _k(1, 1, 0, 0, 0, 0, 0.75), _k(768, 1, 0, 320, 240, 0, 0.75),
                      _k(450, 1.01, 0.2, 321, 239, 0.22, 0.11)),        # value[0] -> ALPHA (slot 6), value[1] -> XI (slot 5)
    "EXTENDED_UNIFIED": (6, _k(1, 1, 0, 0, 0, 0.5, 1.0), _k(768, 1, 0, 320, 240, 0.5, 1.0), _k(450, 1.01, 0.2, 321, 239, 0.11, 0.22)),
    "ORTHOGRAPHIC": (7, _k(1, 1), _k(768, 1, 0, 320, 240), _k(450, 1.01, 0.2, 321, 239, 0.11, 0.22)),
}


@pytest.mark.parametrize("name", sorted(PRIOR_CASES))
def test_intrinsics_from_prior(name):
    model, nothing, size_only, everything = PRIOR_CASES[name]
    m, k = camera.IntrinsicsFromPrior(_prior(name))
    assert m == model and k.shape == (10,) and np.array_equal(k, nothing)
    p = _prior(name)
    p.image_width, p.image_height = 640, 480
    assert np.array_equal(camera.IntrinsicsFromPrior(p)[1], size_only)
    p.image_height = 0                      # one side alone is no size
    assert np.array_equal(camera.IntrinsicsFromPrior(p)[1], nothing)
    assert np.array_equal(camera.IntrinsicsFromPrior(_everything(name))[1], everything)


def test_intrinsics_from_prior_details():
    # 1.2 max(w, h) takes the larger side whichever it is
    p = _prior("PINHOLE"); p.image_width, p.image_height = 480, 640
    assert np.array_equal(camera.IntrinsicsFromPrior(p)[1], _k(768, 1, 0, 240, 320))
    # the twoview module's prior has no tangential field: read as not set
    p = twoview.CameraIntrinsicsPrior(); p.camera_intrinsics_model_type = "PINHOLE_RADIAL_TANGENTIAL"
    assert np.array_equal(camera.IntrinsicsFromPrior(p)[1], _k(1, 1))
    # FOV and the division model write their default back over nothing: the same values
    with pytest.raises(capi.TheiaHipError) as e:
        p = _prior("EQUIRECTANGULAR"); camera.IntrinsicsFromPrior(p)
    assert e.value.code == INV


# ------------------------------------------------------------------ 4. the ABI
def _call(num_obs=1, obs_uv=True, obs_cam=None, num_cameras=1, cam_group=(0,), cam_ext=None, num_groups=1, intrinsics=True,
          group_model=(0,), want=("camera_point",), n_alloc=4):
    """theia_hip_unproject with sentinel-filled outputs -> (return code, the outputs).  True: a valid array; None: NULL."""
    uv = np.full((n_alloc, 2), 3.0) if obs_uv is True else obs_uv
    cam = None if obs_cam is None else np.ascontiguousarray(obs_cam, np.int32)
    grp = None if cam_group is None else np.ascontiguousarray(cam_group, np.int32)
    ext = None if cam_ext is None else np.ascontiguousarray(cam_ext, np.float64)
    intr = np.tile(_k(100, 1, 0, 1, 1), (max(1, num_groups if num_groups > 0 else 1), 1)) if intrinsics is True else intrinsics
    mod = None if group_model is None else np.ascontiguousarray(group_model, np.int32)
    out = {name: np.full((n_alloc, w), -7.0) for name, w in (("camera_point", 3), ("normalized", 2), ("world_ray", 3), ("world_ray_unit", 3))}
    out["status"] = np.full(n_alloc, 77, np.uint8); out["iterations"] = np.full(n_alloc, 77, np.uint8)
    s = capi.UnprojectSummary(); s.num_invalid = -7
    g = lambda name, t: capi.ptr(out[name] if name in want else None, t)
    rc = capi.lib().theia_hip_unproject(
        num_obs, capi.ptr(uv, C.c_double), capi.ptr(cam, C.c_int32), num_cameras, capi.ptr(grp, C.c_int32), capi.ptr(ext, C.c_double),
        num_groups, capi.ptr(intr, C.c_double), capi.ptr(mod, C.c_int32), g("camera_point", C.c_double), g("normalized", C.c_double),
        g("world_ray", C.c_double), g("world_ray_unit", C.c_double), g("status", C.c_uint8), g("iterations", C.c_uint8), C.byref(s))
    out["summary"] = s
    return rc, out


def _untouched(out):
    return all((out[n] == -7.0).all() for n in ("camera_point", "normalized", "world_ray", "world_ray_unit")) and \
        (out["status"] == 77).all() and (out["iterations"] == 77).all() and out["summary"].num_invalid == -7


ALL = ("camera_point", "normalized", "world_ray", "world_ray_unit", "status", "iterations")
REFUSALS = {
    "negative num_obs": dict(num_obs=-1),
    "negative num_cameras": dict(num_cameras=-1),
    "negative num_groups": dict(num_groups=-1),
    "null obs_uv": dict(obs_uv=None),
    "null cam_group": dict(cam_group=None),
    "null intrinsics": dict(intrinsics=None),
    "null group_model": dict(group_model=None),
    "camera index too large": dict(num_obs=2, obs_cam=(0, 1)),
    "camera index negative": dict(num_obs=2, obs_cam=(0, -1)),
    "no camera 0": dict(num_cameras=0, cam_group=None),
    "group index too large": dict(cam_group=(1,)),
    "group index negative": dict(cam_group=(-1,)),
    "group of an unobserved camera": dict(num_cameras=2, cam_group=(0, 5)),
    "model 8": dict(group_model=(8,)),
    "model -1": dict(group_model=(-1,)),
    "world_ray without cam_ext": dict(want=("world_ray",)),
    "world_ray_unit without cam_ext": dict(want=ALL),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_before_the_device(case):
    rc, out = _call(**REFUSALS[case])
    assert rc == INV, case
    assert _untouched(out)
    assert capi.lib().theia_hip_last_error() != b""


def test_refusals_precede_the_empty_call():
    # num_obs == 0 returns 0 -- but not with a negative count or a bad model next to it
    assert _call(num_obs=0, num_cameras=-1)[0] == INV
    assert _call(num_obs=0, group_model=(9,))[0] == INV


def test_header_declaration_matches_the_ctypes_signature():
    src = open(os.path.join(ROOT, "include", "theia_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+theia_hip_unproject\s*\(([^)]*)\)\s*;", src)
    assert m, "theia_hip_unproject is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "const double*": capi.c_double_p, "double*": capi.c_double_p,
             "const int32_t*": capi.c_int32_p, "uint8_t*": capi.c_uint8_p,
             "theia_unproject_summary*": C.POINTER(capi.UnprojectSummary)}
    declared = [ctype[p.rsplit(" ", 1)[0]] for p in params]
    names = [p.rsplit(" ", 1)[1] for p in params]
    assert names == ["num_obs", "obs_uv", "obs_cam", "num_cameras", "cam_group", "cam_ext", "num_groups", "intrinsics",
                     "group_model", "camera_point", "normalized", "world_ray", "world_ray_unit", "status", "iterations", "summary"]
    fn = capi.lib().theia_hip_unproject
    assert list(fn.argtypes) == declared
    assert fn.restype is C.c_int
    assert "theia_hip_unproject" in capi.EXPORTED_SYMBOLS
    # theia_unproject_summary: two int64, two int32, two doubles
    body = re.search(r"typedef struct theia_unproject_summary\s*\{(.*?)\}", src, flags=re.S).group(1)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int64_t num_invalid", "int64_t num_not_converged", "int32_t max_iterations", "int32_t reserved",
                      "double kernel_ms", "double call_ms"]
    assert [n for n, _ in capi.UnprojectSummary._fields_] == [f.split()[1] for f in fields]
    assert C.sizeof(capi.UnprojectSummary) == 2 * 8 + 2 * 4 + 2 * 8


def test_python_mirror_checks_its_arguments():
    with pytest.raises(capi.TheiaHipError) as e:
        camera.unproject(np.zeros((2, 2)), [0], [0], None, _k(1, 1), [0])
    assert e.value.code == INV
    with pytest.raises(capi.TheiaHipError) as e:
        camera.unproject(np.zeros((2, 2)), None, [0], None, _k(1, 1), [0], outputs=("bearing",))
    assert e.value.code == INV
    with pytest.raises(capi.TheiaHipError) as e:      # the C entry's refusal, through the mirror
        camera.unproject(np.zeros((2, 2)), None, [0], None, _k(1, 1), [0], outputs=("world_ray",))
    assert e.value.code == INV
