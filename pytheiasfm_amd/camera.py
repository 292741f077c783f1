"""Pixels -> camera coordinates, normalised features and world rays for all eight camera models, on the device
(theia_hip_unproject, csrc/unproject.hip): Camera::PixelToNormalizedCoordinates / Camera::PixelToUnitDepthRay
(sfm/camera/camera.cc:218-230) for arrays of observations.

The calls here produce the arrays the other mirrors already accept: NormalizedFeatures() is the `normalized_features` of
LocalizeViewToReconstruction, LocalizeViewsToReconstruction, LiGTPositionEstimator, LinearPositionEstimator,
NonlinearPositionEstimator and EstimateTriangulation; ObservationRays() is the `obs_ray_dir` of ba.estimate_tracks.  Those
mirrors keep refusing the non-pinhole models when the argument is left out.
"""
import ctypes as C

import numpy as np

from . import _capi as capi

# camera_intrinsics_model_type.h:46-56, :59-80
MODEL_IDS = {"PINHOLE": 0, "PINHOLE_RADIAL_TANGENTIAL": 1, "FISHEYE": 2, "FOV": 3, "DIVISION_UNDISTORTION": 4,
             "DOUBLE_SPHERE": 5, "EXTENDED_UNIFIED": 6, "ORTHOGRAPHIC": 7}
STATUS_VALID, STATUS_CONVERGED = 1, 2
_OUTPUTS = ("camera_point", "normalized", "world_ray", "world_ray_unit", "status", "iterations")
_WIDTH = {"camera_point": 3, "normalized": 2, "world_ray": 3, "world_ray_unit": 3}


def unproject(obs_uv, obs_cam, cam_group, cam_ext, intrinsics, group_model, outputs=("camera_point", "normalized"),
              summary=False):
    """theia_hip_unproject on arrays laid out as theia_ba_problem's.  obs_cam None: every pixel belongs to camera 0; cam_ext
    None: allowed while no world ray is asked for.  outputs: the names to compute, out of camera_point [n][3], normalized
    [n][2], world_ray [n][3], world_ray_unit [n][3], status [n] uint8 (STATUS_* bits), iterations [n] uint8.  Returns a dict
    of them, plus "summary" (counts and times) when summary is set."""
    for name in outputs:
        if name not in _OUTPUTS:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"unknown output {name!r}")
    uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2)
    n = uv.shape[0]
    cam = None if obs_cam is None else np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    if cam is not None and cam.shape[0] != n:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "one camera index per pixel expected")
    group = np.ascontiguousarray(cam_group, dtype=np.int32).reshape(-1)
    ext = None if cam_ext is None else np.ascontiguousarray(cam_ext, dtype=np.float64).reshape(-1, 6)
    if ext is not None and ext.shape[0] != group.shape[0]:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "one extrinsics row per camera expected")
    model = np.ascontiguousarray(group_model, dtype=np.int32).reshape(-1)
    k = np.asarray(intrinsics, dtype=np.float64)
    k = k.reshape(1, -1) if k.ndim == 1 else k
    if k.shape[0] != model.shape[0] or k.shape[1] > capi.THEIA_MAX_INTRINSICS:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "one intrinsics row of at most 10 per group expected")
    intr = np.zeros((k.shape[0], capi.THEIA_MAX_INTRINSICS))
    intr[:, :k.shape[1]] = k
    out = {}
    for name in outputs:
        out[name] = np.empty((n, _WIDTH[name])) if name in _WIDTH else np.empty(n, dtype=np.uint8)
    s = capi.UnprojectSummary() if summary else None
    dp = lambda name: capi.ptr(out.get(name), C.c_double)
    bp = lambda name: capi.ptr(out.get(name), C.c_uint8)
    capi.check(capi.lib().theia_hip_unproject(
        n, capi.ptr(uv, C.c_double), capi.ptr(cam, C.c_int32), group.shape[0], capi.ptr(group, C.c_int32),
        capi.ptr(ext, C.c_double), model.shape[0], capi.ptr(intr, C.c_double), capi.ptr(model, C.c_int32),
        dp("camera_point"), dp("normalized"), dp("world_ray"), dp("world_ray_unit"), bp("status"), bp("iterations"),
        C.byref(s) if summary else None))
    if summary:
        out["summary"] = s.as_dict()
    return out


def _of_camera(camera, pixels, outputs):
    """One ransac.Camera (position, orientation, intrinsics, model) and an [n][2] array of its pixels."""
    ext = np.concatenate([camera.position, camera.orientation]).reshape(1, 6)
    return unproject(pixels, None, [0], ext, camera.intrinsics, [camera.model], outputs)


def PixelToNormalizedCoordinates(camera, pixels):
    """Camera::PixelToNormalizedCoordinates (camera.cc:228-230) of every pixel -> [n][3]."""
    return _of_camera(camera, pixels, ("camera_point",))["camera_point"]


def PixelToUnitDepthRay(camera, pixels):
    """Camera::PixelToUnitDepthRay (camera.cc:218-226) of every pixel -> [n][3] (not normalised, as in the reference)."""
    return _of_camera(camera, pixels, ("world_ray",))["world_ray"]


def NormalizedFeatures(reconstruction):
    """PixelToNormalizedCoordinates(pixel).hnormalized() of every observation -> [num_obs][2], row for row with
    reconstruction.obs_uv."""
    r = reconstruction
    return unproject(r.obs_uv, r.obs_view, r.view_group, None, r.group_intrinsics, r.group_model, ("normalized",))["normalized"]


def ObservationRays(problem_or_reconstruction):
    """The unit world ray of every observation -> [num_obs][3]: ba.estimate_tracks' obs_ray_dir.  Takes a FlatProblem or an
    sfm.Reconstruction."""
    p = problem_or_reconstruction
    if hasattr(p, "obs_view"):
        args = (p.obs_uv, p.obs_view, p.view_group, p.cam_ext, p.group_intrinsics, p.group_model)
    else:
        args = (p.obs_uv, p.obs_cam, p.cam_group, p.cam_ext, p.intrinsics, p.group_model)
    return unproject(*args, outputs=("world_ray_unit",))["world_ray_unit"]


def IntrinsicsFromPrior(prior):
    """SetFromCameraIntrinsicsPriors of the prior's model on a default-constructed model (*_camera_model.cc) ->
    (THEIA_CAM_* id, intrinsics [10] in the C-ABI's layout).  Host code."""
    name = prior.camera_intrinsics_model_type
    if name not in MODEL_IDS:
        raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"unknown camera model {name!r} (reference: LOG(FATAL))")
    model = MODEL_IDS[name]
    no_skew = name in ("FOV", "DIVISION_UNDISTORTION")          # [f a cx cy d] instead of [f a s cx cy d..]
    k = np.zeros(capi.THEIA_MAX_INTRINSICS)
    k[0] = 1.0                                                   # the constructors: focal 1, aspect 1, skew 0, pp 0
    k[1] = 1.0
    cx = 2 if no_skew else 3
    dist = cx + 2
    if name == "FOV":
        k[dist] = 0.75                                           # kDefaultOmega (fov_camera_model.h:144)
    elif name == "DOUBLE_SPHERE":
        k[6] = 0.75                                              # XI (5) = 0, ALPHA (6) = 0.75 (double_sphere_camera_model.cc:62-63)
    elif name == "EXTENDED_UNIFIED":
        k[5], k[6] = 0.5, 1.0                                    # ALPHA, BETA (extended_unified_camera_model.cc:62-63)
    have_size = prior.image_width != 0.0 and prior.image_height != 0.0
    if prior.focal_length.is_set:
        k[0] = prior.focal_length.value[0]
    elif have_size:                                              # fisheye_camera_model.cc:84: 0.4, every other model 1.2
        k[0] = (0.4 if name == "FISHEYE" else 1.2) * float(max(prior.image_width, prior.image_height))
    if prior.principal_point.is_set:
        k[cx], k[cx + 1] = prior.principal_point.value[0], prior.principal_point.value[1]
    elif have_size:
        k[cx], k[cx + 1] = prior.image_width / 2.0, prior.image_height / 2.0
    if prior.aspect_ratio.is_set:
        k[1] = prior.aspect_ratio.value[0]
    if not no_skew and prior.skew.is_set:
        k[2] = prior.skew.value[0]
    radial = prior.radial_distortion
    if name in ("FOV", "DIVISION_UNDISTORTION"):                 # these two write their default back when the prior is unset
        k[dist] = radial.value[0] if radial.is_set else (0.75 if name == "FOV" else 0.0)
    elif radial.is_set:
        if name == "DOUBLE_SPHERE":                              # value[0] -> ALPHA (slot 6), value[1] -> XI (slot 5): .cc:102-106
            k[6], k[5] = radial.value[0], radial.value[1]
        else:
            count = {"PINHOLE": 2, "ORTHOGRAPHIC": 2, "EXTENDED_UNIFIED": 2, "PINHOLE_RADIAL_TANGENTIAL": 3, "FISHEYE": 4}[name]
            k[5:5 + count] = radial.value[:count]
    tangential = getattr(prior, "tangential_distortion", None)
    if name == "PINHOLE_RADIAL_TANGENTIAL" and tangential is not None and tangential.is_set:
        k[8], k[9] = tangential.value[0], tangential.value[1]
    return model, k


def NormalizeFeatures(prior1, prior2, correspondences):
    """estimate_twoview_info.cc:67-102 for any two camera models: [n][4] pixel correspondences -> [n][4]
    hnormalized(PixelToNormalizedCoordinates); when either focal length prior is missing both focal lengths are reset to 1.
    One device call for both columns."""
    c = np.ascontiguousarray(correspondences, dtype=np.float64).reshape(-1, 4)
    (m1, k1), (m2, k2) = IntrinsicsFromPrior(prior1), IntrinsicsFromPrior(prior2)
    if not prior1.focal_length.is_set or not prior2.focal_length.is_set:
        k1[0] = 1.0
        k2[0] = 1.0
    n = c.shape[0]
    cam = np.tile(np.array([0, 1], dtype=np.int32), n)         # the rows of c.reshape(2n, 2) alternate feature1, feature2
    out = unproject(c.reshape(-1, 2), cam, [0, 1], None, np.stack([k1, k2]), [m1, m2], ("normalized",))
    return out["normalized"].reshape(n, 4)
