// unproject_device.h -- pixel -> camera coordinates of one observation for the eight camera models (gfx950, FP64): the
// inverse of ba_device.h's project().  A restatement of CameraModel::PixelToCameraCoordinates / UndistortPoint of
//   pinhole_camera_model.h:213-300                     pinhole_radial_tangential_camera_model.h:222-362
//   fisheye_camera_model.h:191-341                     fov_camera_model.h:183-305
//   division_undistortion_camera_model.h:232-321       double_sphere_camera_model.h:189-286
//   extended_unified_camera_model.h:189-285            orthographic_camera_model.h:188-274
// operation for operation, in the reference's order: the translation unit that includes this file is compiled with
// -ffp-contract=off, so that + - * / and sqrt give the reference's bits (tan and atan2 are the device library's, a few ulp).
// Intrinsics are in the C-ABI's layout (theia_ba_problem.intrinsics).
#pragma once
#include "ba_device.h"

namespace thip {

struct Unprojected {
  double p[3];      // ImageToCameraCoordinates
  bool valid;       // the model's return value (false: double sphere / extended unified outside their domain)
  bool converged;   // the fixed-point loop left by its break or by the fisheye's early return; closed forms: true
  int trips;        // loop trips run (the one that left included); closed forms: 0
};

// The fixed point of PinholeCameraModel::UndistortPoint (:263-300), shared by the orthographic model (:237-274) with its own
// epsilon: p <- d / (1 + r2 (k1 + k2 r2)).
THIP_DEV void undistort_radial2(double k1, double k2, double dx, double dy, double eps, Unprojected& o) {
  double x = dx, y = dy;
  o.converged = false;
  int i = 0;
  while (i < 100) {
    ++i;
    const double px = x, py = y;
    const double r2 = x * x + y * y;
    const double d = 1.0 + r2 * (k1 + k2 * r2);
    x = dx / d;
    y = dy / d;
    if (fabs(x - px) < eps && fabs(y - py) < eps) { o.converged = true; break; }
  }
  o.trips = i;
  o.p[0] = x; o.p[1] = y; o.p[2] = 1.0;
}

// MODELS: the camera models this instance carries (bit = THEIA_CAM_*), as for project(): an instance without the FOV and
// fisheye models sheds the constants of tan / atan2.  A model outside MODELS (or outside 0..7) gives valid = false.
template <unsigned MODELS = kModelsAll>
THIP_DEV void pixel_to_camera(int model, const double* __restrict__ k, double u, double v, Unprojected& o) {
  if (model < 0 || model > 7 || !((MODELS >> model) & 1u)) model = -1;
  o.valid = true; o.converged = true; o.trips = 0;
  o.p[0] = 0.0; o.p[1] = 0.0; o.p[2] = 1.0;
  // the normalisation of the five models with a skew slot and depth division: y first, then x with the skew removed
  double dx = 0.0, dy = 0.0;
  if (model == THEIA_CAM_PINHOLE || model == THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL || model == THEIA_CAM_FISHEYE ||
      model == THEIA_CAM_DOUBLE_SPHERE || model == THEIA_CAM_EXTENDED_UNIFIED) {
    const double fy = k[0] * k[1];
    dy = (v - k[4]) / fy;
    dx = (u - k[3] - dy * k[2]) / k[0];
  }
  switch (model) {
    case THEIA_CAM_PINHOLE:
      if constexpr ((MODELS >> THEIA_CAM_PINHOLE) & 1u) undistort_radial2(k[5], k[6], dx, dy, 1e-10, o);
      break;
    case THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL:
      if constexpr ((MODELS >> THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL) & 1u) {
        // :298-362  [.., k1 k2 k3 t1 t2]
        const double k1 = k[5], k2 = k[6], k3 = k[7], t1 = k[8], t2 = k[9];
        double x = dx, y = dy;
        o.converged = false;
        int i = 0;
        while (i < 100) {
          ++i;
          const double px = x, py = y;
          const double r2 = x * x + y * y;
          const double rd = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
          const double tx = t2 * (r2 + 2.0 * x * x) + 2.0 * t1 * x * y;
          const double ty = t1 * (r2 + 2.0 * y * y) + 2.0 * t2 * x * y;
          x = (dx - tx) / rd;
          y = (dy - ty) / rd;
          if (fabs(x - px) < 1e-10 && fabs(y - py) < 1e-10) { o.converged = true; break; }
        }
        o.trips = i;
        o.p[0] = x; o.p[1] = y;
      }
      break;
    case THEIA_CAM_FISHEYE:
      if constexpr ((MODELS >> THEIA_CAM_FISHEYE) & 1u) {
        // :274-341  [.., k1 k2 k3 k4]; the early return hands back the DISTORTED point
        const double k1 = k[5], k2 = k[6], k3 = k[7], k4 = k[8];
        double x = dx, y = dy;
        o.converged = false;
        int i = 0;
        while (i < 100) {
          ++i;
          const double px = x, py = y;
          const double r2 = x * x + y * y;
          const double r = sqrt(r2);
          if (r < 1e-8) { x = dx; y = dy; o.converged = true; break; }
          const double th = atan2(r, 1.0);
          const double t2 = th * th;
          const double thd = th * (1.0 + k1 * t2 + k2 * t2 * t2 + k3 * t2 * t2 * t2 + k4 * t2 * t2 * t2 * t2);
          x = r * dx / thd;
          y = r * dy / thd;
          if (fabs(x - px) < 1e-10 && fabs(y - py) < 1e-10) { o.converged = true; break; }
        }
        o.trips = i;
        o.p[0] = x; o.p[1] = y;
      }
      break;
    case THEIA_CAM_FOV:
      if constexpr ((MODELS >> THEIA_CAM_FOV) & 1u) {
        // :183-206, :260-305  [f a cx cy omega]: no skew slot, closed form
        const double fy = k[0] * k[1];
        dx = (u - k[2]) / k[0];
        dy = (v - k[3]) / fy;
        const double omega = k[4];
        const double rd2 = dx * dx + dy * dy;
        double ru;
        if (omega < 1e-3) {
          ru = (omega * omega * rd2) / 3.0 - omega * omega / 12.0 + 1.0;
        } else if (rd2 < 1e-3) {
          ru = (omega * (omega * omega * rd2 + 3.0)) / (6.0 * tan(omega / 2.0));
        } else {
          const double rd = sqrt(rd2);
          ru = tan(rd * omega) / (2.0 * rd * tan(omega / 2.0));
        }
        o.p[0] = ru * dx; o.p[1] = ru * dy;
      }
      break;
    case THEIA_CAM_DIVISION_UNDISTORTION:
      if constexpr ((MODELS >> THEIA_CAM_DIVISION_UNDISTORTION) & 1u) {
        // :232-260, :299-321  [f a cx cy k]: the undistortion acts on the centred PIXEL, the focal lengths divide afterwards
        const double fy = k[0] * k[1];
        dx = u - k[2];
        dy = v - k[3];
        const double rd2 = dx * dx + dy * dy;
        const double undistortion = 1.0 / (1.0 + k[4] * rd2);
        double x = dx * undistortion, y = dy * undistortion;
        x /= k[0];
        y /= fy;
        o.p[0] = x; o.p[1] = y;
      }
      break;
    case THEIA_CAM_DOUBLE_SPHERE:
      if constexpr ((MODELS >> THEIA_CAM_DOUBLE_SPHERE) & 1u) {
        // :251-286  XI is slot 5, ALPHA slot 6
        const double xi = k[5], alpha = k[6];
        const double r2 = dx * dx + dy * dy;
        if (alpha > 0.5 && r2 >= 1.0 / (2.0 * alpha - 1.0)) { o.valid = false; break; }
        const double xi2_2 = alpha * alpha;
        const double xi1_2 = xi * xi;
        const double sqrt2 = sqrt(1.0 - (2.0 * alpha - 1.0) * r2);
        const double norm2 = alpha * sqrt2 + 1.0 - alpha;
        const double mz = (1.0 - xi2_2 * r2) / norm2;
        const double mz2 = mz * mz;
        const double norm1 = mz2 + r2;
        const double sqrt1 = sqrt(mz2 + (1.0 - xi1_2) * r2);
        const double kk = (mz * xi + sqrt1) / norm1;
        o.p[0] = kk * dx; o.p[1] = kk * dy; o.p[2] = kk * mz - xi;
      }
      break;
    case THEIA_CAM_EXTENDED_UNIFIED:
      if constexpr ((MODELS >> THEIA_CAM_EXTENDED_UNIFIED) & 1u) {
        // :251-285  ALPHA is slot 5, BETA slot 6; a unit vector
        const double alpha = k[5], beta = k[6];
        const double r2 = dx * dx + dy * dy;
        const double gamma = 1.0 - alpha;
        if (alpha > 0.5 && r2 >= 1.0 / ((alpha - gamma) * beta)) { o.valid = false; break; }
        const double tmp1 = 1.0 - alpha * alpha * beta * r2;
        const double tmp_sqrt = sqrt(1.0 - (alpha - gamma) * beta * r2);
        const double tmp2 = alpha * tmp_sqrt + gamma;
        const double kk = tmp1 / tmp2;
        double norm = sqrt(r2 + kk * kk);
        if (norm < 1e-12) norm = 1e-12;
        o.p[0] = dx / norm; o.p[1] = dy / norm; o.p[2] = kk / norm;
      }
      break;
    case THEIA_CAM_ORTHOGRAPHIC:
      if constexpr ((MODELS >> THEIA_CAM_ORTHOGRAPHIC) & 1u) {
        // :188-215: the skew is removed BEFORE the division by fx, fy; the pinhole fixed point with epsilon 1e-16 (:241)
        const double fy = k[0] * k[1];
        dy = v - k[4];
        dx = u - k[3] - dy * k[2];
        dx /= k[0];
        dy /= fy;
        undistort_radial2(k[5], k[6], dx, dy, 1e-16, o);
      }
      break;
    default:
      o.valid = false;
      break;
  }
}

}  // namespace thip
