// BundleAdjuster::GetCovarianceForViews / GetCovarianceForTracks on a problem with variable cameras AND variable tracks
// (theia_hip_ba_covariance_full behind the shim), checked against the same blocks asked for through the C-ABI directly on a
// handle at the adjusted state, and for the shape of a partially constant camera's block.
// Prints "ok coupled covariances" and exits non-zero on failure (tests/test_shim_covariance_full.py runs it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bundle_adjuster_hip.h"

using namespace theia_hip_shim;

static void rotate(const double w[3], const double p[3], double out[3]) {   // Rodrigues
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 < 1e-30) { for (int i = 0; i < 3; ++i) out[i] = p[i]; return; }
  const double th = std::sqrt(th2), c = std::cos(th), s = std::sin(th);
  const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
  const double kxp[3] = {k[1] * p[2] - k[2] * p[1], k[2] * p[0] - k[0] * p[2], k[0] * p[1] - k[1] * p[0]};
  const double kp = k[0] * p[0] + k[1] * p[1] + k[2] * p[2];
  for (int i = 0; i < 3; ++i) out[i] = p[i] * c + kxp[i] * s + k[i] * kp * (1 - c);
}

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  const int nv = 6, nt = 80;
  std::vector<double> cam(6 * nv), cam_true(6 * nv), pts(4 * nt), pts_true(4 * nt);
  double intr[7] = {800.0, 1.0, 0.0, 500.0, 400.0, 0.0, 0.0};
  for (int v = 0; v < nv; ++v) {
    double* e = &cam_true[6 * v];
    e[0] = 4.0 * std::cos(0.9 * v) + 0.2 * U(gen); e[1] = 0.3 * U(gen); e[2] = -8.0 + 0.5 * U(gen);
    e[3] = 0.05 * U(gen); e[4] = -0.12 * std::cos(0.9 * v); e[5] = 0.05 * U(gen);
  }
  for (int t = 0; t < nt; ++t) { pts_true[4 * t] = 3 * U(gen); pts_true[4 * t + 1] = 2 * U(gen); pts_true[4 * t + 2] = 2 * U(gen); pts_true[4 * t + 3] = 1.0; }
  cam = cam_true; pts = pts_true;
  for (int v = 1; v < nv; ++v) for (int q = 3; q < 6; ++q) cam[6 * v + q] += 0.01 * N(gen);
  for (int v = 2; v < nv; ++v) for (int q = 0; q < 3; ++q) cam[6 * v + q] += 0.05 * N(gen);
  for (int t = 0; t < nt; ++t) for (int q = 0; q < 3; ++q) pts[4 * t + q] += 0.05 * N(gen);

  BundleAdjustmentOptions opts;
  opts.max_num_iterations = 30;
  BundleAdjuster ba(opts);
  ba.AddIntrinsicsGroup(0, THEIA_CAM_PINHOLE, intr, 7);
  for (int v = 0; v < nv; ++v) ba.AddCamera(v, &cam[6 * v], 0);
  for (int t = 0; t < nt; ++t) ba.AddTrack(t, &pts[4 * t]);
  std::vector<double> uvs; std::vector<int32_t> oc, op;
  const double cov[2] = {1.0, 1.0};
  for (int t = 0; t < nt; ++t)
    for (int v = 0; v < nv; ++v) {
      if (((t * 31 + v * 17) % 5) > 2) continue;
      const double* e = &cam_true[6 * v];
      const double d[3] = {pts_true[4 * t] - e[0], pts_true[4 * t + 1] - e[1], pts_true[4 * t + 2] - e[2]};
      double q[3];
      rotate(e + 3, d, q);
      if (q[2] <= 0.1) continue;
      const double uv[2] = {intr[0] * q[0] / q[2] + intr[3] + 0.3 * N(gen), intr[0] * intr[1] * q[1] / q[2] + intr[4] + 0.3 * N(gen)};
      ba.AddObservation(v, t, uv, cov);
      uvs.push_back(uv[0]); uvs.push_back(uv[1]); oc.push_back(v); op.push_back(t);
    }
  ba.SetCameraExtrinsicsConstant(0);   // the classic gauge fix: one camera, one position
  ba.SetCameraPositionConstant(1);
  const BundleAdjustmentSummary s = ba.Optimize();
  if (!ba.error().empty() || !s.success) { std::printf("FAIL: bundle adjustment %s\n", ba.error().c_str()); return 1; }

  const std::vector<ViewId> views = {1, 4};
  const std::vector<TrackId> tracks = {0, 33, 79};
  std::vector<std::vector<double>> cv, ct;
  if (!ba.GetCovarianceForViews(views, &cv) || !ba.GetCovarianceForTracks(tracks, &ct)) { std::printf("FAIL: %s\n", ba.error().c_str()); return 1; }
  if (cv.size() != 2 || ct.size() != 3 || cv[0].size() != 36 || ct[0].size() != 9) { std::printf("FAIL: sizes\n"); return 1; }

  // the same blocks through the C-ABI on a handle at the adjusted state
  std::vector<uint8_t> cc(nv, 0), pc(nt, 0);
  cc[0] = THEIA_CAM_CONST_ALL; cc[1] = THEIA_CAM_CONST_POSITION;
  std::vector<int32_t> cam_group(nv, 0), model(1, THEIA_CAM_PINHOLE);
  std::vector<double> k(THEIA_MAX_INTRINSICS, 0.0), si(uvs.size(), 1.0);
  std::memcpy(k.data(), intr, sizeof(intr));
  theia_ba_problem P;
  std::memset(&P, 0, sizeof(P));
  P.num_cameras = nv; P.num_groups = 1; P.num_points = nt; P.num_obs = (int64_t)oc.size();
  P.cam_ext = cam.data(); P.intrinsics = k.data(); P.group_model = model.data(); P.cam_group = cam_group.data();
  P.cam_const = cc.data(); P.points = pts.data(); P.point_const = pc.data();
  P.obs_uv = uvs.data(); P.obs_sqrt_info = si.data(); P.obs_cam = oc.data(); P.obs_pt = op.data();
  theia_ba_options O;
  theia_ba_options_default(&O);
  theia_ba_handle h = nullptr;
  if (theia_hip_ba_create(&P, &O, &h) != THEIA_HIP_OK) { std::printf("FAIL: %s\n", theia_hip_last_error()); return 1; }
  std::vector<double> all_c(36 * nv), all_p(9 * nt);
  const int rc = theia_hip_ba_covariance_full(h, 0, nullptr, 0, nullptr, 0, all_c.data(), all_p.data());
  theia_hip_ba_destroy(h);
  if (rc != THEIA_HIP_OK) { std::printf("FAIL: %s\n", theia_hip_last_error()); return 1; }
  double worst = 0.0;
  for (size_t i = 0; i < views.size(); ++i) {
    double mx = 0.0;
    for (int e = 0; e < 36; ++e) mx = std::fmax(mx, std::fabs(all_c[36 * views[i] + e]));
    if (!(mx > 0.0)) { std::printf("FAIL: empty view block\n"); return 1; }
    for (int e = 0; e < 36; ++e) worst = std::fmax(worst, std::fabs(cv[i][e] - all_c[36 * views[i] + e]) / mx);
  }
  for (size_t i = 0; i < tracks.size(); ++i) {
    double mx = 0.0;
    for (int e = 0; e < 9; ++e) mx = std::fmax(mx, std::fabs(all_p[9 * tracks[i] + e]));
    if (!(mx > 0.0)) { std::printf("FAIL: empty track block\n"); return 1; }
    for (int e = 0; e < 9; ++e) worst = std::fmax(worst, std::fabs(ct[i][e] - all_p[9 * tracks[i] + e]) / mx);
  }
  std::printf("shim against the C-ABI: %.3e relative\n", worst);
  if (!(worst < 1e-9)) { std::printf("FAIL: shim blocks differ from the C-ABI's\n"); return 1; }
  // view 1 has a constant position: zero rows and columns there, a positive diagonal on the rotation
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      const double v = cv[0][6 * a + b];
      if ((a < 3 || b < 3) ? v != 0.0 : (a == b && !(v > 0.0))) { std::printf("FAIL: partially constant camera block\n"); return 1; }
      if (cv[1][6 * a + b] != cv[1][6 * b + a] || (a == b && !(cv[1][6 * a + a] > 0.0))) { std::printf("FAIL: view block\n"); return 1; }
    }
  for (const auto& c : ct)
    if (!(c[0] > 0 && c[4] > 0 && c[8] > 0) || c[1] != c[3] || c[2] != c[6] || c[5] != c[7]) { std::printf("FAIL: track block\n"); return 1; }
  std::printf("ok coupled covariances\n");
  return 0;
}
