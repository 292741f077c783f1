"""Restatement of CameraModel::PixelToCameraCoordinates of the eight camera models and of Camera::PixelToUnitDepthRay
(sfm/camera/*_camera_model.h, camera.cc:218-226), one pixel at a time, in Python floats with math.sqrt / atan2 / tan.
Written from the reference headers; the operation order is the reference's (Python evaluates a * b * c left to right, as
C++ does).  Intrinsics are in the C-ABI's layout.

pixel_to_camera(model, k, u, v) -> ((x, y, z), valid, converged, trips)
    valid: the model's return value; on False the point is (nan, nan, nan), the library's stated deviation
    converged: the fixed-point loop left by its break or by the fisheye's early return; closed forms: True
    trips: loop trips run, the one that left included; closed forms: 0
"""
import math

import numpy as np

NAN3 = (math.nan, math.nan, math.nan)
ITERATIVE = (0, 1, 2, 7)


def _skew_normalised(k, u, v):
    # the y coordinate first, then x with the skew removed (pinhole_camera_model.h:228-232 and its four siblings)
    fy = k[0] * k[1]
    dy = (v - k[4]) / fy
    dx = (u - k[3] - dy * k[2]) / k[0]
    return dx, dy


def _radial2(k1, k2, dx, dy, eps):
    # PinholeCameraModel::UndistortPoint (:263-300); OrthographicCameraModel::UndistortPoint (:237-274) with its epsilon
    x, y = dx, dy
    for i in range(100):
        px, py = x, y
        r_sq = x * x + y * y
        d = 1.0 + r_sq * (k1 + k2 * r_sq)
        x = dx / d
        y = dy / d
        if abs(x - px) < eps and abs(y - py) < eps:
            return (x, y, 1.0), True, True, i + 1
    return (x, y, 1.0), True, False, 100


def pinhole(k, u, v):
    dx, dy = _skew_normalised(k, u, v)
    return _radial2(k[5], k[6], dx, dy, 1e-10)


def pinhole_radial_tangential(k, u, v):
    # :222-251, :298-362
    dx, dy = _skew_normalised(k, u, v)
    k1, k2, k3, t1, t2 = k[5], k[6], k[7], k[8], k[9]
    x, y = dx, dy
    for i in range(100):
        px, py = x, y
        r_sq = x * x + y * y
        rd = 1.0 + k1 * r_sq + k2 * r_sq * r_sq + k3 * r_sq * r_sq * r_sq
        tangential_x = t2 * (r_sq + 2.0 * x * x) + 2.0 * t1 * x * y
        tangential_y = t1 * (r_sq + 2.0 * y * y) + 2.0 * t2 * x * y
        x = (dx - tangential_x) / rd
        y = (dy - tangential_y) / rd
        if abs(x - px) < 1e-10 and abs(y - py) < 1e-10:
            return (x, y, 1.0), True, True, i + 1
    return (x, y, 1.0), True, False, 100


def fisheye(k, u, v):
    # :191-219, :274-341
    dx, dy = _skew_normalised(k, u, v)
    k1, k2, k3, k4 = k[5], k[6], k[7], k[8]
    x, y = dx, dy
    for i in range(100):
        px, py = x, y
        r_sq = x * x + y * y
        r = math.sqrt(r_sq)
        if r < 1e-8:
            return (dx, dy, 1.0), True, True, i + 1      # the distorted point
        theta = math.atan2(r, 1.0)
        theta_sq = theta * theta
        theta_d = theta * (1.0 + k1 * theta_sq + k2 * theta_sq * theta_sq + k3 * theta_sq * theta_sq * theta_sq +
                           k4 * theta_sq * theta_sq * theta_sq * theta_sq)
        x = r * dx / theta_d
        y = r * dy / theta_d
        if abs(x - px) < 1e-10 and abs(y - py) < 1e-10:
            return (x, y, 1.0), True, True, i + 1
    return (x, y, 1.0), True, False, 100


def fov_branch(k, u, v):
    """0: omega < 1e-3, 1: r_d^2 < 1e-3, 2: the tan form."""
    dx = (u - k[2]) / k[0]
    dy = (v - k[3]) / (k[0] * k[1])
    if k[4] < 1e-3:
        return 0
    return 1 if dx * dx + dy * dy < 1e-3 else 2


def fov(k, u, v):
    # :183-206, :260-305  [f a cx cy omega]
    fy = k[0] * k[1]
    dx = (u - k[2]) / k[0]
    dy = (v - k[3]) / fy
    omega = k[4]
    r_d_sq = dx * dx + dy * dy
    if omega < 1e-3:
        r_u = (omega * omega * r_d_sq) / 3.0 - omega * omega / 12.0 + 1.0
    elif r_d_sq < 1e-3:
        r_u = (omega * (omega * omega * r_d_sq + 3.0)) / (6.0 * math.tan(omega / 2.0))
    else:
        r_d = math.sqrt(r_d_sq)
        r_u = math.tan(r_d * omega) / (2.0 * r_d * math.tan(omega / 2.0))
    return (r_u * dx, r_u * dy, 1.0), True, True, 0


def division_undistortion(k, u, v):
    # :232-260, :299-321  [f a cx cy k]
    fy = k[0] * k[1]
    dx = u - k[2]
    dy = v - k[3]
    r_d_sq = dx * dx + dy * dy
    undistortion = 1.0 / (1.0 + k[4] * r_d_sq)
    x = dx * undistortion
    y = dy * undistortion
    x /= k[0]
    y /= fy
    return (x, y, 1.0), True, True, 0


def double_sphere(k, u, v):
    # :189-212, :251-286  XI = slot 5, ALPHA = slot 6
    dx, dy = _skew_normalised(k, u, v)
    xi, alpha = k[5], k[6]
    r2 = dx * dx + dy * dy
    if alpha > 0.5:
        if r2 >= 1.0 / (2.0 * alpha - 1.0):
            return NAN3, False, True, 0
    xi2_2 = alpha * alpha
    xi1_2 = xi * xi
    sqrt2 = math.sqrt(1.0 - (2.0 * alpha - 1.0) * r2)
    norm2 = alpha * sqrt2 + 1.0 - alpha
    mz = (1.0 - xi2_2 * r2) / norm2
    mz2 = mz * mz
    norm1 = mz2 + r2
    sqrt1 = math.sqrt(mz2 + (1.0 - xi1_2) * r2)
    kk = (mz * xi + sqrt1) / norm1
    return (kk * dx, kk * dy, kk * mz - xi), True, True, 0


def extended_unified(k, u, v):
    # :189-212, :251-285  ALPHA = slot 5, BETA = slot 6
    dx, dy = _skew_normalised(k, u, v)
    alpha, beta = k[5], k[6]
    r2 = dx * dx + dy * dy
    gamma = 1.0 - alpha
    if alpha > 0.5:
        if r2 >= 1.0 / ((alpha - gamma) * beta):
            return NAN3, False, True, 0
    tmp1 = 1.0 - alpha * alpha * beta * r2
    tmp_sqrt = math.sqrt(1.0 - (alpha - gamma) * beta * r2)
    tmp2 = alpha * tmp_sqrt + gamma
    kk = tmp1 / tmp2
    norm = math.sqrt(r2 + kk * kk)
    if norm < 1e-12:
        norm = 1e-12
    return (dx / norm, dy / norm, kk / norm), True, True, 0


def orthographic(k, u, v):
    # :188-215: the skew before the division; epsilon 1e-16 (:241)
    fy = k[0] * k[1]
    dy = v - k[4]
    dx = u - k[3] - dy * k[2]
    dx /= k[0]
    dy /= fy
    return _radial2(k[5], k[6], dx, dy, 1e-16)


_MODELS = (pinhole, pinhole_radial_tangential, fisheye, fov, division_undistortion, double_sphere, extended_unified,
           orthographic)


def pixel_to_camera(model, k, u, v):
    k = [float(x) for x in k] + [0.0] * 10
    return _MODELS[model](k, float(u), float(v))


def angle_axis_to_rotation_matrix(w):
    """ceres::AngleAxisToRotationMatrix (rotation.h), row-major R as Camera::GetOrientationAsRotationMatrix returns it."""
    theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if theta2 > np.finfo(np.float64).eps:
        theta = math.sqrt(theta2)
        wx, wy, wz = w[0] / theta, w[1] / theta, w[2] / theta
        c, s = math.cos(theta), math.sin(theta)
        return [[c + wx * wx * (1.0 - c), wx * wy * (1.0 - c) - wz * s, wy * s + wx * wz * (1.0 - c)],
                [wz * s + wx * wy * (1.0 - c), c + wy * wy * (1.0 - c), -wx * s + wy * wz * (1.0 - c)],
                [-wy * s + wx * wz * (1.0 - c), wx * s + wy * wz * (1.0 - c), c + wz * wz * (1.0 - c)]]
    return [[1.0, -w[2], w[1]], [w[2], 1.0, -w[0]], [-w[1], w[0], 1.0]]


def pixel_to_unit_depth_ray(model, k, angle_axis, u, v):
    """Camera::PixelToUnitDepthRay (camera.cc:218-226): R' * PixelToNormalizedCoordinates(pixel)."""
    p = pixel_to_camera(model, k, u, v)[0]
    R = angle_axis_to_rotation_matrix([float(x) for x in angle_axis])
    return tuple(R[0][j] * p[0] + R[1][j] * p[1] + R[2][j] * p[2] for j in range(3))


def unproject(model, k, pixels):
    """Every pixel of an [n][2] array -> dict of camera_point [n][3], normalized [n][2], status [n], iterations [n]."""
    pixels = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    n = pixels.shape[0]
    out = {"camera_point": np.empty((n, 3)), "normalized": np.empty((n, 2)), "status": np.empty(n, np.uint8),
           "iterations": np.empty(n, np.uint8)}
    for i in range(n):
        p, valid, converged, trips = pixel_to_camera(model, k, pixels[i, 0], pixels[i, 1])
        out["camera_point"][i] = p
        out["normalized"][i] = (p[0] / p[2], p[1] / p[2]) if valid else (math.nan, math.nan)
        out["status"][i] = (1 if valid else 0) | (2 if converged else 0)
        out["iterations"][i] = trips
    return out
