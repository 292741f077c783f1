// ba_host_rules.h -- the host-side rules every BA path applies to a flat problem (ba_plan.hip, ba_solver.hip, ba_invdepth.hip):
// which intrinsics a model frees, how many it has, the bounds of its initial point, and the camera priors in use.
#pragma once
#include <algorithm>
#include <vector>

#include "theia_hip.h"

namespace thip {

// Free intrinsics of a model under an OptimizeIntrinsicsType mask
// (GetSubsetFromOptimizeIntrinsicsType of every *_camera_model.cc, e.g.
// pinhole_camera_model.cc:132-162): bit q = parameter q is optimised.
inline unsigned intrinsics_free_mask(int model, int opt) {
  const bool noskew = (model == THEIA_CAM_FOV || model == THEIA_CAM_DIVISION_UNDISTORTION);
  unsigned m = 0;
  if (opt & THEIA_INTR_FOCAL_LENGTH) m |= 1u << 0;
  if (opt & THEIA_INTR_ASPECT_RATIO) m |= 1u << 1;
  if ((opt & THEIA_INTR_SKEW) && !noskew) m |= 1u << 2;
  if (opt & THEIA_INTR_PRINCIPAL_POINTS) m |= noskew ? (3u << 2) : (3u << 3);
  if (opt & THEIA_INTR_RADIAL_DISTORTION) {
    switch (model) {
      case THEIA_CAM_PINHOLE: case THEIA_CAM_DOUBLE_SPHERE: case THEIA_CAM_EXTENDED_UNIFIED: case THEIA_CAM_ORTHOGRAPHIC: m |= 3u << 5; break;
      case THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL: m |= 7u << 5; break;
      case THEIA_CAM_FISHEYE: m |= 15u << 5; break;
      case THEIA_CAM_FOV: case THEIA_CAM_DIVISION_UNDISTORTION: m |= 1u << 4; break;
    }
  }
  if ((opt & THEIA_INTR_TANGENTIAL_DISTORTION) && model == THEIA_CAM_PINHOLE_RADIAL_TANGENTIAL) m |= 3u << 8;
  return m;
}
inline int intrinsics_size(int model) {
  static const int K[8] = {7, 10, 9, 5, 5, 7, 7, 7};  // kIntrinsicsSize of the eight models
  return (model >= 0 && model < 8) ? K[model] : 0;
}
// bundle_adjuster.cc:406-427 parameter bounds (applied to the initial point as Ceres does)
inline void project_intrinsics_to_bounds(int model, double* k) {
  if (k[0] < 1.0) k[0] = 1.0;
  if (model == THEIA_CAM_DOUBLE_SPHERE) { k[5] = std::min(1.0, std::max(-1.0, k[5])); k[6] = std::min(1.0, std::max(0.0, k[6])); }
  if (model == THEIA_CAM_EXTENDED_UNIFIED) { k[5] = std::min(1.0, std::max(0.0, k[5])); k[6] = std::max(0.1, k[6]); }
}
// camera priors in use: the camera's bit AND the option's bit (bundle_adjuster.cc:159-172,291-313), of the cameras with
// used[c] != 0 (null: of all); appends camera, kind, the 3-vector and the 3 x 3 square-root information of each
inline void collect_cam_priors(const theia_ba_problem* p, int prior_mask, int nc, const uint8_t* used, std::vector<int>& pc,
                               std::vector<int>& pk, std::vector<double>& pv, std::vector<double>& pi) {
  if (!p->cam_prior_mask || !prior_mask) return;
  const double* vecs[3] = {p->cam_position_prior, p->cam_gravity_prior, p->cam_orientation_prior};
  const double* infos[3] = {p->cam_position_prior_sqrt_info, p->cam_gravity_prior_sqrt_info, p->cam_orientation_prior_sqrt_info};
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < 3; ++k) {
      const int bit = 1 << k;
      if ((used && !used[c]) || !(p->cam_prior_mask[c] & bit) || !(prior_mask & bit) || !vecs[k] || !infos[k]) continue;
      pc.push_back(c); pk.push_back(bit);
      pv.insert(pv.end(), vecs[k] + 3 * (size_t)c, vecs[k] + 3 * (size_t)c + 3);
      pi.insert(pi.end(), infos[k] + 9 * (size_t)c, infos[k] + 9 * (size_t)c + 9);
    }
}

}  // namespace thip
